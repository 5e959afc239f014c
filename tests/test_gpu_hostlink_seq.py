"""Sequenced payloads on the host link (mpx_xfer_hostlink_seq /
mpx_host_xfer_seq, include/mpx_hostlink_seq.h) on the real kernels (-m gpu).

One GPU rank and one endpoint on threads unless noted (tests/hostlink_seq.py).
Every expectation is host bytes: oracle_py.fill under mpx.pattern_key and
oracle_py.checksum of those bytes.  After every call both ends' whole rx and
tx are compared byte for byte, the call's counts and digest with numbers
recomputed on the host, and every link counter of both ends with what an
ordinary host-link call moves.  Calls under an MPX_TEST knob or a forced
MPX_HOSTLINK_LL run in a process of their own (tests/hostlink_seq_worker.py).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import hostlink_duplex
import hostlink_seq as S
import mpx
import payload
from hostlink import M64, P31, P32, LinkMap
from hostlink_seq import BIG, LINK, PP, UNI
from seq import SEED, csum

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = [PP, UNI]
GROUPS = [1, 0]          # the GPU rank's group: 1 = it sends first (unidir: it sends the payload)
SIZES = [0, 1, 8, 255, 256, 257, 2045, 4161, BIG]
G, E = LINK

_maps = {}


def one(n: int) -> LinkMap:
    """GPU rank 0 and endpoint 1: one map for the sizes up to 4161 B, one for the large one"""
    key = 4161 if n <= 4161 else n
    if key not in _maps:
        _maps[key] = S.one(key)
    return _maps[key]


@pytest.fixture(scope="module", autouse=True)
def _close_maps():
    yield
    for h in _maps.values():
        h.close()
    _maps.clear()


@pytest.fixture(autouse=True)
def _a_failed_map_is_not_reused(request):
    failed = request.session.testsfailed
    yield
    if request.session.testsfailed != failed:
        _maps.clear()      # (left open: a side may still be inside its call)


def worker(cases, **env_extra):
    env = dict(os.environ, **env_extra)
    for k in ("MPX_HOSTLINK_LL", "MPX_HOSTLINK_WG"):
        if k not in env_extra:
            env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "hostlink_seq_worker.py"), json.dumps(cases)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(got) == len(cases), got
    return got


# ---- 1. the matrix ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_every_iteration_delivers_its_own_payload(mode, gpu_group, n):
    """both modes and orientations, both forms either side of the 256-byte
    threshold, one workgroup, several with a tail, the default cap of 16; 1, 2,
    3 and 33 iterations: checked against host expectations, with the
    library's own (2 iterations) and unchecked (3)"""
    assert mpx.hostlink_ll_max() == 256
    h = one(n)
    for iters, check, expect in ((1, True, "host"), (2, True, None), (3, False, "host"), (33, True, "host")):
        out = S.call(h, mode, gpu_group, n, iters, check=check, expect=expect, what=("matrix", mode, gpu_group, n, iters))
        width = 1 if n <= 256 else payload.chunk_shape(min(16, max(1, -(-n // 32768))), n)[0]
        assert [out[G].nwg, out[E].nwg] == [width, width], (n, out[G].nwg, out[E].nwg)


# ---- 2. widths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nwg,n", [(7, 4161), (70, 71681)])
@pytest.mark.parametrize("gpu_group", GROUPS)
def test_explicit_widths_both_directions_bulk(gpu_group, nwg, n):
    """width 7 at 4161 B (narrowed to 5) and width 70 at 71 681 B (an empty chunk)"""
    h = one(n)
    out = S.call(h, PP, gpu_group, n, 5, nwg=nwg, what=("width", nwg, n))
    assert out[G].nwg == out[E].nwg == payload.chunk_shape(nwg, n)[0]
    out = S.call(h, UNI, gpu_group, n, 5, nwg=nwg, what=("width uni", nwg, n))
    assert out[G].nwg == out[E].nwg == payload.chunk_shape(nwg, n)[0]


# ---- 3. forced forms ----------------------------------------------------------------------------
def test_threshold_0_makes_everything_bulk():
    """MPX_HOSTLINK_LL=0 in a child process: the 8-byte payload and the unidir
    ack are pulled (the endpoint writes them into tx) and pushed as bulk
    messages; 0 bytes stay LL.  Verified in full by the worker."""
    cases = [dict(mode=m, gpu_group=g, n=n, iters=5, check=1, full=1) for m in MODES for g in GROUPS for n in (0, 8)]
    got = worker(cases, MPX_HOSTLINK_LL="0")
    for c, r in zip(cases, got):
        assert r["verified"] and r["protocol"] == (mpx.PROTO_HOSTLINK_BULK if c["n"] else mpx.PROTO_HOSTLINK_LL), (c, r)


def test_threshold_8192_makes_8_kib_ll_messages():
    cases = [dict(mode=m, gpu_group=g, n=8185, iters=5, check=1, full=1) for m in MODES for g in GROUPS]
    got = worker(cases, MPX_HOSTLINK_LL="8192")
    for c, r in zip(cases, got):
        assert r["verified"] and r["protocol"] == mpx.PROTO_HOSTLINK_LL and r["nwg"] == [1, 1], (c, r)


# ---- 4. every pulled payload is fresh -----------------------------------------------------------
FRESH = [(UNI, 0), (PP, 0), (PP, 1)]      # (mode, the GPU rank's group): the endpoint sends the n bytes


@pytest.mark.parametrize("n", [4161, BIG])
@pytest.mark.parametrize("mode,gpu_group", FRESH)
def test_every_pulled_payload_is_fresh(mode, gpu_group, n):
    """33 checked iterations whose payload the GPU pulls across the link from
    a tx the endpoint rewrites before every send: no check fails"""
    out = S.call(one(n), mode, gpu_group, n, 33, what=("fresh", mode, gpu_group, n))
    assert out[G].check_failures == 0 and out[G].check_iters == 33


@pytest.mark.parametrize("k", [2, 17, 33])
def test_a_stale_payload_fails_the_gpus_check_at_its_iteration(k):
    """MPX_TEST=seq_stale=k in a child process: the endpoint's k-th send
    repeats the payload before it (a bulk send leaves tx unwritten, an LL send
    packs the key before).  The call completes; the GPU side returns
    MPX_ERR_CHECK with exactly one failure, the endpoint's side is clean.  The
    failing iteration is exactly k - 1: the same call passes once expect[k - 1]
    is the checksum of payload k - 2.  For k = iters the unchecked call's rx
    holds payload iters - 2.  LL sizes fail alike.
    Without the sequenced loop nothing here can fail: these are the controls."""
    iters = 33
    shapes = [(m, g, n) for (m, g) in FRESH for n in (4161, BIG)] + [(UNI, 0, 8), (PP, 0, 255), (PP, 1, 8)]
    cases = []
    for m, g, n in shapes:
        base = dict(mode=m, gpu_group=g, n=n, iters=iters)
        cases.append(dict(base, check=1))
        cases.append(dict(base, check=1, alt=["gpu", k - 1, "payload", k - 2]))
        if k == iters:
            cases.append(dict(base, check=0, rx_gpu=["payload", iters - 2]))
    got = worker(cases, MPX_TEST=f"seq_stale={k}")
    clean = {"status": mpx.OK, "check_failures": 0, "check_iters": iters, "recv_done": iters}
    for c, r in zip(cases, got):
        if not c["check"]:
            assert r["gpu"]["status"] == r["host"]["status"] == mpx.OK and r["rx_gpu_ok"], (c, r)
        elif "alt" in c:
            assert r["gpu"] == clean and r["host"] == clean, (c, r)
        else:
            assert r["gpu"] == dict(clean, status=mpx.ERR_CHECK, check_failures=1), (c, r)
            assert r["host"] == clean, (c, r)


def test_a_stale_first_send_sends_what_tx_held():
    """seq_stale=1: the first send has no predecessor; the GPU receives the
    bytes the endpoint's tx was seeded with, in both forms"""
    cases = []
    for n in (8, 4161):
        base = dict(mode=UNI, gpu_group=0, n=n, iters=3)
        cases += [dict(base, check=1), dict(base, check=1, alt=["gpu", 0, "tx", 0])]
    got = worker(cases, MPX_TEST="seq_stale=1")
    clean = {"status": mpx.OK, "check_failures": 0, "check_iters": 3, "recv_done": 3}
    for c, r in zip(cases, got):
        want = clean if "alt" in c else dict(clean, status=mpx.ERR_CHECK, check_failures=1)
        assert r["gpu"] == want and r["host"] == clean, (c, r)


# ---- 5. lost payloads ---------------------------------------------------------------------------
def test_a_lost_payload_fails_the_receivers_check_at_iteration_1():
    """MPX_TEST=skip_push=2 in a child process, each direction and form: the
    receiver's check fails once, the sender's side is clean, nothing times
    out.  The failing iteration is 1: the call passes once expect[1] is the
    checksum of what a lost payload leaves behind (LL from the GPU: the tags
    with ff data; LL from the endpoint: zero data; bulk: iteration 0's poison,
    5a in every byte)."""
    shapes = [("gpu", 1, 8, 0xFF), ("gpu", 1, 4161, 0x5A), ("host", 0, 8, 0x00), ("host", 0, 4161, 0x5A)]
    cases = []
    for sender, gpu_group, n, left in shapes:
        receiver = "host" if sender == "gpu" else "gpu"
        base = dict(mode=UNI, gpu_group=gpu_group, n=n, iters=5)
        cases += [dict(base, check=1), dict(base, check=1, alt=[receiver, 1, "byte", left]), dict(base, check=0)]
    got = worker(cases, MPX_TEST="skip_push=2")
    clean = {"status": mpx.OK, "check_failures": 0, "check_iters": 5, "recv_done": 5}
    for c, r in zip(cases, got):
        receiver = "gpu" if c["gpu_group"] == 0 else "host"
        sender = "host" if receiver == "gpu" else "gpu"
        if not c["check"]:
            assert r["gpu"]["status"] == r["host"]["status"] == mpx.OK, (c, r)
        elif "alt" in c:
            assert r[receiver] == clean and r[sender] == clean, (c, r)
        else:
            assert r[receiver] == dict(clean, status=mpx.ERR_CHECK, check_failures=1), (c, r)
            assert r[sender] == clean, (c, r)


# ---- 6. across 2^31 and 2^32 --------------------------------------------------------------------
@pytest.mark.parametrize("P", [P31, P32])
def test_a_checked_call_across(P):
    """links that start 4 pushes short of P (mpx_test_advance_link on both
    ends, token_by 0), the boundary inside a 9-iteration checked call, LL and
    bulk, both modes and orientations — every case on a link of its own (an LL
    row must not have held tags 2^31 pushes back)"""
    shapes = [(m, g, n) for m in MODES for g in GROUPS for n in (8, 4161)]
    h = LinkMap(4161, 1 + len(shapes), [0], range(1, 1 + len(shapes)), [(0, k) for k in range(1, 1 + len(shapes))])
    try:
        for k, (m, g, n) in enumerate(shapes):
            link = (0, 1 + k)
            h.jump(link, P - 4)
            S.call(h, m, g, n, 9, link=link, what=("across", P, m, g, n))
            assert h.counters(*link)["tx_seq"] == P + 4 == h.counters(link[1], link[0])["rx_seq"]
    finally:
        h.close()


# ---- 7. mixed calls on one link -----------------------------------------------------------------
def test_sequenced_ordinary_duplex_and_pair_calls_alternate():
    """on one link: sequenced, ordinary checked, full duplex, a pair call of the
    GPU rank with a second GPU rank, sequenced again under another seed"""
    n = 4161
    h = LinkMap(n, 3, [0, 2], [1], [LINK])
    try:
        for mode, g in ((PP, 1), (UNI, 0)):
            S.call(h, mode, g, n, 5, what="mixed: sequenced")
            h.set_tx(E, 0x717171 + g)               # (the sequenced call wrote the endpoint's tx)
            h.call([LINK], mode, g, n, 4, what="mixed: ordinary")
            hostlink_duplex.call(h, [LINK], n, 6, what="mixed: duplex")
            h.pair(0, 2, PP, n, 3, what="mixed: pair")
            S.call(h, mode, g, n, 5, seed=SEED ^ 0xABCDEF, what="mixed: sequenced, another seed")
            S.call(h, mode, g, 8, 5, what="mixed: sequenced LL")
            h.call([LINK], mode, g, 8, 4, what="mixed: ordinary LL")
    finally:
        h.close()


# ---- 8. one-sided -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 4161])
@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_only_the_gpu_side_sequenced(mode, gpu_group, n):
    """unchecked: both calls return OK; the GPU's rx holds the endpoint's tx
    bytes, the endpoint's rx the GPU's last generated payload, and the
    endpoint's tx is untouched (its ordinary call does not write it)"""
    h = one(n)
    iters = 4

    def go():
        S.prepare(h)
        out, errs = S.run(h, LINK, mode, gpu_group, n, iters, check=False, seq_sides=("gpu",))
        assert not errs, {k: str(x) for k, x in errs.items()}
        return out
    out = h.counted([LINK], iters, go, "one-sided")
    m_gpu, m_host = S.lens(mode, gpu_group, n)[1], S.lens(mode, 1 - gpu_group, n)[1]
    payload.compare(h.rx(G), h.tx_bytes[E][:m_gpu] + h.blank()[m_gpu:], 0, "one-sided: the GPU's rx")
    payload.compare(h.rx(E), S.want_rx(h, G, E, m_host, iters - 1), 0, "one-sided: the endpoint's rx")
    payload.compare(h.tx(E), h.tx_bytes[E], 0, "one-sided: the endpoint's tx")
    payload.compare(h.tx(G), h.tx_bytes[G], 0, "one-sided: the GPU's tx")
    assert out[G].recv_done == out[E].recv_done == iters


# ---- 9. the recorder ----------------------------------------------------------------------------
def test_a_sequenced_call_leaves_the_recorder_alone():
    h = S.one(4161)
    try:
        for r in LINK:
            h.c.hostlink_lat_enable(r, 16)
        h.call([LINK], PP, 1, 4161, 6, what="recorder: a traced call")
        before = {r: h.c.hostlink_lat_get(r, p) for r, p in ((G, E), (E, G))}
        assert all(b["count"] == 6 and b["calls"] == 1 for b in before.values()), before
        raw = {r: h.c.hostlink_lat_raw(r, p) for r, p in ((G, E), (E, G))}
        for n in (4161, 8):
            S.call(h, PP, 1, n, 5, what="recorder: sequenced")
            S.call(h, UNI, 0, n, 5, what="recorder: sequenced")
        assert {r: h.c.hostlink_lat_get(r, p) for r, p in ((G, E), (E, G))} == before
        assert {r: h.c.hostlink_lat_raw(r, p) for r, p in ((G, E), (E, G))} == raw
    finally:
        h.close()


# ---- 10. refusals -------------------------------------------------------------------------------
def test_refusals_come_before_any_gpu_work():
    """each refusal: its status, a zeroed mpx_timing, no counter of any rank moved"""
    n = 4161
    h = LinkMap(n, 4, [0, 2], [1], [LINK])        # rank 3 stays unattached
    try:
        c = h.c
        tx, rx = h.gpu[0]

        def gpu(mode=PP, me=0, host=1, iters=3, flags=0, check=False, expect=None, bufs=None):
            return lambda: c.xfer_hostlink_seq(mode, 1, me, host, iters, *(bufs or h.gpu[0]), n, SEED, check_payload=check,
                                               expect=expect, flags=flags, timeout_ms=2000)

        def host(mode=PP, me=1, peer=0, iters=3, flags=0, check=False, expect=None):
            return lambda: c.host_xfer_seq(mode, 0, me, peer, iters, n, SEED, check_payload=check, expect=expect,
                                           flags=flags, timeout_ms=2000)
        over = (mpx.SEQ_AUTO_MAX // n) + 1
        cases = [("non-blocking", gpu(mode=mpx.MODE_NONBLOCKING), mpx.ERR_UNSUPPORTED),
                 ("non-blocking, endpoint", host(mode=mpx.MODE_NONBLOCKING), mpx.ERR_UNSUPPORTED),
                 ("NOSTAGE", gpu(flags=mpx.XFER_NOSTAGE), mpx.ERR_INVALID),
                 ("STREAM", gpu(flags=mpx.XFER_STREAM), mpx.ERR_INVALID),
                 ("another bit", gpu(flags=1 << 9), mpx.ERR_INVALID),
                 ("NOSTAGE, endpoint", host(flags=mpx.XFER_NOSTAGE), mpx.ERR_INVALID),
                 ("STREAM, endpoint", host(flags=mpx.XFER_STREAM), mpx.ERR_INVALID),
                 ("the host rank is a GPU rank", gpu(host=2), mpx.ERR_INVALID),
                 ("the host rank is unattached", gpu(host=3), mpx.ERR_INVALID),
                 ("my rank is the endpoint", gpu(me=1, host=1), mpx.ERR_INVALID),
                 ("my rank is unattached", gpu(me=3), mpx.ERR_INVALID),
                 ("the endpoint's peer is an endpoint", host(peer=1), mpx.ERR_INVALID),
                 ("the endpoint is a GPU rank", host(me=2), mpx.ERR_INVALID),
                 ("rank out of range", gpu(host=4), mpx.ERR_INVALID),
                 ("another rank's buffers", gpu(bufs=h.gpu[2]), mpx.ERR_INVALID),
                 ("expect NULL above the cap", gpu(iters=over, check=True), mpx.ERR_INVALID),
                 ("expect NULL above the cap, endpoint", host(iters=over, check=True), mpx.ERR_INVALID)]
        was = h.all_counters()
        for what, fn, status in cases:
            with pytest.raises(mpx.MpxError) as x:
                fn()
            assert x.value.status == status, (what, x.value.status, str(x.value))
            assert bytes(x.value.timing) == bytes(C.sizeof(mpx.Timing)), what
            assert h.all_counters() == was, what
        # NULL opts: the raw call
        t = mpx.Timing()
        C.memset(C.byref(t), 0xFF, C.sizeof(t))
        L = mpx.lib()
        assert L.mpx_xfer_hostlink_seq(c.h, PP, 1, 0, 1, 3, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr), n, None,
                                       C.byref(t)) == mpx.ERR_INVALID
        assert L.mpx_host_xfer_seq(c.h, PP, 0, 1, 0, 3, n, None, C.byref(t)) == mpx.ERR_INVALID
        assert h.all_counters() == was
        # an armed rank: MPX_ERR_STATE, and the armed call is still there to disarm
        c.arm(PP, 1, 0, 2, 3, tx, rx, n, timeout_ms=2000)
        armed = h.all_counters()
        with pytest.raises(mpx.MpxError) as x:
            gpu()()
        assert x.value.status == mpx.ERR_STATE and bytes(x.value.timing) == bytes(C.sizeof(mpx.Timing))
        assert h.all_counters() == armed
        c.disarm(0)
        # and the link works
        S.call(h, PP, 1, n, 3, what="after the refusals")
    finally:
        h.close()


# ---- 11. mpx_perf -H -K 1 -----------------------------------------------------------------------
@pytest.mark.parametrize("args,n,iters,runs,check,proto", [
    (["-H", "1", "-K", "1", "-c", "1", "-b", "4161", "-i", "7", "-r", "3"], 4161, 7, 3, True, "host_bulk"),
    (["-H", "2", "-K", "1", "-u", "1", "-b", "8", "-i", "5"], 8, 5, None, False, "host_ll")])
def test_mpx_perf_runs_sequenced_host_link_calls(tmp_path, args, n, iters, runs, check, proto):
    """exit 0, a record and a side line per run after the first, every payload
    of a -c 1 run checked; the digest is the host's, from the run's seed"""
    from test_gpu_host import run
    p, recs, side = run(tmp_path, args + ["-w", "1", "-f", "@G1", "-n", "1", "-p", "1", "-l", "@LOGS"] +
                        ([] if runs else ["-r", "3"]), gpus="0")
    assert p.returncode == 0, p.stderr[-800:]
    assert len(recs) == 2 and len(side) == 2
    h2 = args[1] == "2"
    writer, peer = (1, 0) if h2 else (0, 1)           # the group-1 rank holds the logs
    for x in side:
        run_idx = int(x[17])
        assert (int(x[2]), int(x[6]), int(x[8]), int(x[9]), x[13]) == (writer, peer, n, iters, proto), x
        m = 1 if "-u" in args else n                  # (the group-1 side of a unidir run receives the ack)
        assert int(x[18]) == iters and int(x[16]) == 0, x
        if check:
            seed = (mpx.PATTERN_SEED + run_idx * 0x9E3779B97F4A7C15) & M64
            assert int(x[15]) == iters, x
            assert int(x[19]) == sum(csum(seed, peer, writer, i, m) for i in range(iters)) & M64, x
        else:
            assert int(x[15]) == 0, x
