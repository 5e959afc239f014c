"""The host link's full-duplex loop on the GPU (include/mpx_hostlink_duplex.h):
a GPU rank and a CPU endpoint run the reference's non-blocking loop across the
PCIe link, both directions at once.  One GPU.  Every expectation is host bytes
(tests/hostlink.py: oracle_py.fill seeds tx, oracle_py.checksum sums it) or the
compiled reference's fixture (tests/golden/ref_runs.json), never the library's
own output.  Buffers are attached 4 KiB longer than the message and rx starts
as 0xEE; both ends' whole rx and tx are compared after both sides have
returned, and every counter of every attached rank after every call.  No time
is asserted anywhere; every wait of every case is bounded (timeout_ms <= 5000
and the helper's join limit), and each case runs once.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import mpx
import oracle_py as O
import payload
import hostlink_duplex as D
from hostlink import M64, P32, LinkMap

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BIG = (256 << 10) + 21
PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
GOLDEN = {c["name"]: c for c in O.golden()["cases"]}

_maps = {}


def link_map(n: int) -> LinkMap:
    """GPU rank 0 and endpoint 1 with buffers for messages of n bytes, shared by the cases of that size"""
    if n not in _maps:
        _maps[n] = D.one_gpu(n)
    return _maps[n]


def drop(n: int) -> None:
    h = _maps.pop(n, None)
    if h is not None:
        h.close()


@pytest.fixture(scope="module", autouse=True)
def _close_maps():
    yield
    for n in list(_maps):
        drop(n)


def call(n_map: int, n: int, iters: int, check: bool, **kw):
    """a call on the shared map of that size; a map that failed is not reused"""
    h = link_map(n_map)
    try:
        return D.call(h, h.links, n, iters, check=check, **kw)
    except BaseException:
        _maps.pop(n_map, None)   # (a side may still run: the context is left alone)
        raise


# ---- sizes ------------------------------------------------------------------------
# (n, width asked for, staged): 0, 1, 8 and 17 B go through the bulk form at
# width 1 (17: one unit and a tail); 1024 against 1025 at width 2 is one
# workgroup against two per direction; BIG at the default width (9), at 7
# (ragged) and with MPX_XFER_NOSTAGE; 71681 at width 70 has an empty chunk
SHAPES = [(0, 0, True), (1, 0, True), (8, 0, True), (17, 0, True), (1024, 2, True), (1025, 2, True), (4161, 0, True),
          (BIG, 0, True), (BIG, 7, True), (BIG, 0, False), (71681, 70, True)]


@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n,nwg,stage", SHAPES)
def test_sizes(n, nwg, stage, iters, check):
    assert [D.width(*s[:2]) for s in SHAPES] == [1, 1, 1, 1, 1, 2, 1, 9, 7, 9, 70]
    assert payload.chunk_shape(70, 71681) == (70, 1040, 1, 68, 961) and payload.chunk_shape(7, BIG)[1] * 7 != BIG
    call(BIG if n > 4161 else 4161, n, iters, check, nwg=nwg, stage=stage, what=("sizes", n, nwg, stage))


# ---- iteration counts: the publish schedule (15, 16, 17) and the window ----------------
@pytest.mark.parametrize("check", [False, True])
@pytest.mark.parametrize("iters", [15, 16, 17, 254, 255, 256, 257, 512, 600])
@pytest.mark.parametrize("n", [64, 4161])
def test_iteration_counts(n, iters, check):
    """recv_done = iters - iters // 256, check_iters = iters and recv_digest over
    the counted receives, on both ends (hostlink_duplex.verify)"""
    assert [D.counted_receives(i) for i in (254, 255, 256, 257, 512, 600)] == [254, 255, 255, 256, 510, 598]
    call(4161, n, iters, check, what=("iterations", n, iters))


@pytest.mark.parametrize("iters", [255, 256, 257, 512, 600])
def test_receive_accounting_matches_the_reference(iters):
    """The configuration of golden nonblocking_window_i* (64 B, the
    reference's 'b' / 'a' fill, its -r runs) with the GPU rank in reference
    rank 0's place and the endpoint in rank 1's: each end's summed recv_done,
    bytes and recv_digest equal what the compiled reference's ranks received
    (the PMPI shim's entries).  The method of
    test_gpu_engine.py::test_receive_digest_matches_reference; the numbers
    come from the compiled reference."""
    c = GOLDEN[f"nonblocking_window_i{iters}"]
    a = c["args"]
    assert int(a[a.index("-i") + 1]) == iters and int(a[a.index("-b") + 1]) == 64 and "-x" in a and c["np"] == 2
    runs = int(a[a.index("-r") + 1])
    h = link_map(4161)
    g, e = h.links[0]
    try:
        for r, byte in ((g, b"b"), (e, b"a")):        # mpi_perf.c:244-251: group 1 sends 'b', group 0 'a'
            h.tx_bytes[r] = byte * h.cap
            if r == g:
                payload.write(h.c, h.gpu[g][0], h.tx_bytes[r])
            else:
                C.memmove(h.host[e][0], h.tx_bytes[r], h.cap)
        total = {g: [0, 0, 0], e: [0, 0, 0]}
        for _ in range(runs):
            out = call(4161, 64, iters, True, what=("reference", iters))
            for r in (g, e):
                t = out[(g, e), r]
                assert t.check_failures == 0 and t.check_iters == iters
                total[r][0] += t.recv_done
                total[r][1] += t.recv_done * 64
                total[r][2] = (total[r][2] + t.recv_digest) & M64
        for r, ref_rank in ((g, "0"), (e, "1")):
            ref = c["shim"][ref_rank]
            assert total[r] == [ref["recv_done"], ref["recv_bytes"], ref["recv_digest"]], (r, total[r], ref)
    finally:
        drop(4161)      # (its tx no longer holds the seeded bytes)


def _worker(args, env_extra, drop_env=()):
    env = dict(os.environ, **env_extra)
    for k in drop_env:
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "hostlink_duplex_worker.py"), *args], capture_output=True,
                       text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("every", ["1", "2", "256"])
def test_publish_schedule(every):
    """MPX_NB_PUBLISH (read once per process) at its ends: every push and
    receive published, every other one, and none but slot 254 and the last —
    600 iterations of 4161 B at width 3, unchecked and checked, verified in
    the worker against host bytes"""
    got = _worker(["publish"], {"MPX_NB_PUBLISH": every})
    assert got == {"ok": True, "recv_done": [598] * 4}


# ---- counter wraps -----------------------------------------------------------------
@pytest.mark.parametrize("check", [False, True])
def test_push_numbers_across_2_to_32(check):
    """links whose next push is number 2^32 - 4 on both ends: the boundary
    inside a 33-iteration call, and between two calls; flag, credit and ready
    words, the kernel's relay words and the endpoint's compares all cross it"""
    h = D.one_gpu(4161, 2)
    try:
        for n in (64, 4161):
            inside, between = h.links
            h.jump(inside, P32 - 4)
            D.call(h, [inside], n, 33, check=check, nwg=3, what=("2^32 inside", n))
            assert h.counters(*inside)["tx_seq"] == P32 + 28 == h.counters(inside[1], inside[0])["rx_seq"]
            h.jump(between, P32 - 4)
            D.call(h, [between], n, 4, check=check, nwg=3, what=("2^32 first of two", n))
            assert h.counters(*between)["tx_seq"] == P32 - 1
            D.call(h, [between], n, 4, check=check, nwg=3, what=("2^32 second of two", n))
            assert h.counters(*between)["tx_seq"] == P32 + 3 == h.counters(between[1], between[0])["rx_seq"]
            h.close()
            h = D.one_gpu(4161, 2)
    finally:
        h.close()


def test_call_number_across_2_to_32():
    """a link advanced to 2 calls short of call 2^32: the posted handshake
    across it, with a call without iterations in between (it posts nothing
    and takes no number)"""
    h = D.one_gpu(4161)
    link = g, e = h.links[0]
    try:
        h.advance(link, calls_by=P32 - 2)
        assert h.counters(g, e)["calls"] == h.counters(e, g)["calls"] == P32 - 2
        D.call(h, [link], 4161, 3, check=True, what="call 2^32 - 1")
        D.call(h, [link], 4161, 0, check=True, what="no iterations")
        assert h.counters(g, e)["calls"] == h.counters(e, g)["calls"] == P32 - 1
        D.call(h, [link], 4161, 257, check=True, what="call 2^32")
        D.call(h, [link], 64, 5, check=False, what="call 2^32 + 1")
        assert h.counters(g, e)["calls"] == h.counters(e, g)["calls"] == P32 + 1
    finally:
        h.close()


def test_one_link_through_several_forms():
    """duplex, LL ping-pong, duplex (checked), bulk unidir each way, duplex
    again on ONE link: the blocking forms find the link as a pair call would
    leave it, and the full-duplex loop finds theirs; every counter of both
    ends is asserted after each step (counted)"""
    h = link_map(4161)
    link = h.links[0]
    try:
        D.call(h, [link], 4161, 300, check=False, what="forms: duplex")
        h.call([link], PP, 1, 8, 5, what="forms: LL ping-pong")
        D.call(h, [link], 4161, 20, check=True, nwg=3, what="forms: duplex, checked")
        h.call([link], UNI, 1, 4161, 4, what="forms: bulk unidir, device to host")
        h.call([link], UNI, 0, 4161, 4, what="forms: bulk unidir, host to device")
        D.call(h, [link], 64, 17, check=True, what="forms: duplex again")
        D.call(h, [link], 4161, 0, check=True, what="forms: a call that moves nothing")
        h.call([link], PP, 0, 4161, 3, what="forms: bulk ping-pong")
    except BaseException:
        _maps.pop(4161, None)
        raise


def test_two_links_at_once():
    """two GPU ranks on GPU 0, each with an endpoint of its own, four threads:
    each rank's tx has a seed of its own, so a byte of the other link would show"""
    h = LinkMap(BIG, 4, [0, 1], [2, 3], [(0, 2), (1, 3)])
    try:
        for n, iters, check in ((BIG, 20, False), (4161, 257, True), (BIG, 5, True)):
            D.call(h, h.links, n, iters, check=check, what=("two links", n, iters))
    finally:
        h.close()


@pytest.mark.parametrize("late", ["host", "gpu"])
def test_a_late_side_keeps_its_rx_until_it_calls(late):
    """Call 1, then call 2 which one side enters 0.2 s late.  Read the moment
    before it enters, the late side's rx still holds its prefill (it was reset
    after call 1) although the other side has been in call 2 all along; and
    the early side cannot have returned before the late one entered: each side
    ends only after its sends were taken."""
    h = link_map(4161)
    link = g, e = h.links[0]
    late_rank, early_rank = (e, g) if late == "host" else (g, e)
    try:
        D.call(h, [link], 4161, 3, check=False, what="ordering: call 1")

        def second():
            h.reset_rx()
            out, errs = D.run(h, [link], 4161, 3, check=True, delay={late_rank: 0.2},
                              before={late_rank: lambda: h.rx(late_rank)})
            assert not errs, {k: str(x) for k, x in errs.items()}
            payload.compare(h.seen[late_rank], h.blank(), 0, f"the late {late} side's rx before it entered call 2")
            assert h.returned[early_rank] >= h.entered[late_rank]
            D.verify(h, out, [link], 4161, 3, True, ("ordering", late))
            return out
        h.counted([link], 3, second, ("ordering", late))
    except BaseException:
        _maps.pop(4161, None)
        raise


# ---- a lost payload ------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 4161])
def test_a_lost_payload_fails_both_checks(n):
    """MPX_TEST=skip_push=2 in a process of its own: the 2nd payload of EACH
    direction is lost (the GPU skips the stores of push 2 and the loads of pull
    2; flags and credits still come).  Checked, both ends return MPX_ERR_CHECK
    with exactly one failure each and nothing times out; the same call
    unchecked succeeds unseen."""
    got = _worker(["lost", str(n)], {"MPX_TEST": "skip_push=2"})
    for side in ("gpu", "host"):
        assert got[side] == {"status": mpx.ERR_CHECK, "check_failures": 1, "check_iters": 5, "recv_done": 5}, got
    assert got["unchecked"] == [mpx.OK, mpx.OK], got


@pytest.mark.parametrize("n", [8, 4161])
def test_a_lost_payload_shows_in_the_bytes(n):
    """The unchecked control of the byte comparison.  Every payload of a call
    carries the same bytes (tx must not change during a call), so payload 1
    alone already leaves rx as the whole call would: the 2nd payload's loss
    cannot show in bytes.  The control is therefore skip_push=1 on a
    one-iteration call, as tests/test_gpu_fan.py's: the call succeeds on both
    ends and the comparison of either end's rx raises."""
    got = _worker(["lost_bytes", str(n)], {"MPX_TEST": "skip_push=1"})
    assert got == {"status": [mpx.OK, mpx.OK], "raised": [True, True]}, got


# ---- deadlines: the bounded waits doing their job --------------------------------------
def test_gpu_side_deadline():
    """mpx_xfer_hostlink_duplex alone at five workgroups per direction: the
    pushing half's reader waits for the endpoint's post, the rest for its
    relay; MPX_ERR_TIMEOUT, then MPX_ERR_STATE; the endpoint of that link is
    not broken, and a fresh context works"""
    h = D.one_gpu(8192)
    try:
        with pytest.raises(mpx.MpxError) as ei:
            h.c.xfer_hostlink_duplex(0, 1, 3, *h.gpu[0], 8192, timeout_ms=300, nwg=5)
        assert ei.value.status == mpx.ERR_TIMEOUT
        with pytest.raises(mpx.MpxError) as ei:
            h.c.xfer_hostlink_duplex(0, 1, 3, *h.gpu[0], 8192, timeout_ms=300, nwg=5)
        assert ei.value.status == mpx.ERR_STATE
    finally:
        h.close()
    call(4161, 4161, 3, True, what="after the GPU side's deadline")


@pytest.mark.parametrize("iters", [3, 300])
def test_cpu_side_deadline(iters):
    """mpx_host_xfer_duplex alone (no kernel is launched): its final wait, or
    its first window flush, runs out; MPX_ERR_TIMEOUT, then MPX_ERR_STATE"""
    h = D.one_gpu(4161)
    try:
        with pytest.raises(mpx.MpxError) as ei:
            h.c.host_xfer_duplex(1, 0, iters, 4161, timeout_ms=100)
        assert ei.value.status == mpx.ERR_TIMEOUT
        with pytest.raises(mpx.MpxError) as ei:
            h.c.host_xfer_duplex(1, 0, iters, 4161, timeout_ms=100)
        assert ei.value.status == mpx.ERR_STATE
        payload.compare(h.rx(1), h.blank(), 0, "the endpoint's rx after its deadline")
    finally:
        h.close()


# ---- refusals, each decided before any GPU work or wait ---------------------------------
def test_refusals_on_a_live_context():
    h = link_map(4161)
    c, (tx, rx) = h.c, h.gpu[0]
    L = c.L
    t = mpx.Timing()

    def status(fn, *a, **kw):
        with pytest.raises(mpx.MpxError) as ei:
            fn(*a, **kw)
        return ei.value.status

    was = h.all_counters()
    assert status(c.xfer_hostlink_duplex, 0, 0, 1, tx, rx, 8) == mpx.ERR_INVALID            # host_rank is a GPU rank
    assert status(c.xfer_hostlink_duplex, 1, 1, 1, tx, rx, 8) == mpx.ERR_INVALID            # my_rank is a host endpoint
    assert status(c.host_xfer_duplex, 0, 0, 1, 8) == mpx.ERR_INVALID
    assert status(c.host_xfer_duplex, 1, 1, 1, 8) == mpx.ERR_INVALID
    for my, host in ((-1, 1), (0, 2), (2, 1), (0, -1)):                                     # out of range
        assert status(c.xfer_hostlink_duplex, my, host, 1, tx, rx, 8) == mpx.ERR_INVALID
        assert status(c.host_xfer_duplex, host, my, 1, 8) == mpx.ERR_INVALID
    assert status(c.xfer_hostlink_duplex, 0, 1, -1, tx, rx, 8) == mpx.ERR_INVALID
    assert status(c.host_xfer_duplex, 1, 0, 1, -8) == mpx.ERR_INVALID
    assert status(c.xfer_hostlink_duplex, 0, 1, 1, rx, tx, 8) == mpx.ERR_INVALID            # a foreign tx
    assert L.mpx_xfer_hostlink_duplex(c.h, 0, 1, 1, None, C.c_void_p(rx.ptr), 8, None, C.byref(t)) == mpx.ERR_INVALID
    assert status(c.xfer_hostlink_duplex, 0, 1, 1, tx, rx, h.cap + 1) == mpx.ERR_INVALID    # an over-long buff_len
    assert status(c.host_xfer_duplex, 1, 0, 1, h.cap + 1) == mpx.ERR_INVALID
    for flag in (mpx.XFER_STREAM, mpx.XFER_PULL, mpx.XFER_FAN_LL, mpx.XFER_STREAM | mpx.XFER_NOSTAGE):
        o = mpx.XferOpts(flags=flag)
        assert L.mpx_xfer_hostlink_duplex(c.h, 0, 1, 1, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr), 8, C.byref(o),
                                          C.byref(t)) == mpx.ERR_INVALID
        assert L.mpx_host_xfer_duplex(c.h, 1, 0, 1, 8, C.byref(o), C.byref(t)) == mpx.ERR_INVALID
    assert status(c.xfer_hostlink_duplex, 0, 1, 1, tx, rx, 8, nwg=257) == mpx.ERR_INVALID
    # the blocking entry points go on refusing the non-blocking mode
    assert status(c.xfer_hostlink, mpx.MODE_NONBLOCKING, 1, 0, 1, 1, tx, rx, 8) == mpx.ERR_UNSUPPORTED
    assert status(c.host_xfer, mpx.MODE_NONBLOCKING, 0, 1, 0, 1, 8) == mpx.ERR_UNSUPPORTED
    # an armed GPU rank (armed towards itself: the non-blocking self-pair) refuses the call, and it cannot be armed
    c.arm(mpx.MODE_NONBLOCKING, 1, 0, 0, 1, tx, rx, 8)
    try:
        assert status(c.xfer_hostlink_duplex, 0, 1, 1, tx, rx, 8) == mpx.ERR_STATE
    finally:
        c.disarm(0)
    assert status(c.arm, mpx.MODE_NONBLOCKING, 1, 0, 1, 1, tx, rx, 8) == mpx.ERR_STATE      # (a host endpoint is no pair peer)
    # the latency recorder never traces it: enabled, a duplex call leaves it empty
    c.lat_enable(0)
    try:
        D.call(h, h.links, 4161, 5, check=True, what="traced rank")
        assert c.lat_get(0)["calls"] == 0
    finally:
        c.lat_disable(0)
    # SDMA and RCCL contexts have no host link
    for engine in ("sdma", "rccl"):
        with mpx.Context(2, engine) as c2:
            assert L.mpx_host_xfer_duplex(c2.h, 1, 0, 1, 8, None, C.byref(t)) == mpx.ERR_UNSUPPORTED
            assert L.mpx_xfer_hostlink_duplex(c2.h, 0, 1, 1, None, None, 8, None, C.byref(t)) == mpx.ERR_UNSUPPORTED
    # nothing refused above took a number or moved a byte: the link still works
    now = h.all_counters()
    assert now[0, 1]["tx_seq"] == was[0, 1]["tx_seq"] + 5 and now[1, 0]["calls"] == was[1, 0]["calls"] + 1
    call(4161, 4161, 3, True, what="after the refusals")


def test_a_width_above_128_per_direction_is_refused():
    """129 workgroups per direction would be a grid of 258"""
    n = 129 << 10
    h = D.one_gpu(n)
    try:
        for fn, args in ((h.c.xfer_hostlink_duplex, (0, 1, 1, *h.gpu[0], n)), (h.c.host_xfer_duplex, (1, 0, 1, n))):
            with pytest.raises(mpx.MpxError) as ei:
                fn(*args, nwg=129)
            assert ei.value.status == mpx.ERR_INVALID
        D.call(h, h.links, n, 3, check=True, nwg=128, what="width 128")
    finally:
        h.close()


def test_phases_of_a_duplex_call():
    """mpx_last_phases works for the GPU side as for a pair call"""
    h = link_map(4161)
    D.call(h, h.links, 4161, 9, check=False, what="phases")
    ph = h.c.phases(0)
    assert ph["wall_s"] > 0 and ph["kernel_s"] > 0 and ph["armed"] == 0
    assert 0 < ph["first_iter_s"] <= ph["kernel_s"]


@pytest.mark.parametrize("n,h", [(8, "1"), (4161, "2")])
def test_mpx_perf_full_duplex_runs(tmp_path, n, h):
    """mpx_perf -H -X 1 -c 2: one GPU rank and its endpoint, 257 iterations of
    seeded payloads, every one checked; the records have the reference's shape
    (11 fields, written by group 1's side), the side file names the protocol
    and counts 256 receives; nothing in stderr but the job id, the two INFO
    lines and run 0's summary"""
    from test_gpu_host import run
    p, recs, side = run(tmp_path, ["-H", h, "-X", "1", "-w", "1", "-f", "@G1", "-n", "1", "-p", "1", "-b", str(n), "-i", "257",
                                   "-r", "3", "-c", "2", "-l", "@LOGS"], gpus="0")
    assert p.returncode == 0, p.stderr[-600:]
    writer = 0 if h == "1" else 1
    assert len(recs) == 2 and len(side) == 2
    for f in recs:
        assert len(f) == 11 and int(f[7]) == n and int(f[8]) == 257
    for f in side:
        assert int(f[2]) == writer and int(f[6]) == 1 - writer and f[3] == "kernel" and f[13] == "host_duplex"
        assert int(f[4]) == mpx.MODE_NONBLOCKING
        assert int(f[15]) == 257 and int(f[16]) == 0 and int(f[18]) == 256 and f[20] == "inline"
    lines = [ln for ln in p.stderr.splitlines() if ln.strip()]
    assert len(lines) == 4 and lines[0].startswith("UUID: ") and lines[3].startswith("[Run#: 0]: Total time: "), lines
