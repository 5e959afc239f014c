"""mpx_xfer_fan with MPX_FAN_LL: per link a lock-step exchange of LL granules,
one workgroup per link, pushes double-buffered in the two halves of the
sender's LL row (-m gpu, MI355X; loopback ranks on GPU 0, tests/fan_ll.py).

Every expectation is host bytes: tx is written from the host with distinct
seeded bytes per (src, dst), rx is 0xEE before a call and read back WHOLE after
it (the gaps between blocks, the rank's own block and the blocks of ranks
outside the peer set must still be 0xEE), tx is read back unchanged, digests
are recomputed on the host, and after every call every link's counters are read
from both sides (Fan.counted).  Every deadline is 5000 ms or lower and, but
for the timeout case, none is expected to be used.  All cases fail on a
library without the flag, which answers MPX_ERR_INVALID.
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys
import threading

import pytest

import mpx
import oracle_py as O
import payload
from fan import M64, flat_image, full_mesh, round16
from fan_ll import LL_MAX, PROTO_FAN_LL, LLFan, mesh, race

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "fan_ll_worker.py")
PINGPONG, NONBLOCKING, UNIDIR = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING, mpx.MODE_UNIDIR
P31, P32 = 1 << 31, 1 << 32
Q = 1 << 32
MESH3 = full_mesh(3)
LINKS3 = [(0, 1), (0, 2), (1, 2)]
STAR = {0: [1, 2], 1: [0], 2: [0]}


def worker(args, mpx_test, timeout=60):
    p = subprocess.run([sys.executable, WORKER, *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, MPX_TEST=mpx_test))
    assert p.returncode == 0, (args, p.stdout[-600:], p.stderr[-1500:])
    return json.loads(p.stdout.strip().splitlines()[-1])


# ---- 1. sizes -----------------------------------------------------------------
SIZES = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 4088, 4095, 4096]


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_iteration_counts(n, check):
    """block lengths around the 4-byte granule, the 8-byte word, the 16-byte
    unit, one unit per lane (2048 B = 256 units) and the cap, for 1, 2, 3 and 8
    iterations (both halves, and each reused); three ranks, full mesh; at 9
    bytes also with the blocks a page apart"""
    for stride in [max(16, round16(n))] + ([4096] if n == 9 else []):
        F = mesh(3, n, stride)
        try:
            for k, iters in enumerate((1, 2, 3, 8)):
                if k:
                    F.set_tx_seed(k)
                F.checked_call(MESH3, iters, check, ("sizes", n, stride, iters, check))
        finally:
            F.close()


# ---- 2. a lagging receiver -------------------------------------------------------
LAG_US = 200000


@pytest.mark.parametrize("iters", [4, 5])
@pytest.mark.parametrize("nranks", [2, 3])
def test_a_lagging_receiver(nranks, iters):
    """MPX_TEST=lag_wg=1:0:200000 (a process of its own): rank 1's workgroup of
    its link to rank 0 stalls 0.2 s between its push and its wait of iteration
    iters / 2, while rank 0 has pushed the next iteration already — into the
    other half; a single landing zone would hold that push where rank 1 still
    polls.  The worker verifies bytes, digests and counters (Fan.checked_call).
    Both ends of the lagging link last at least half the injected delay (a
    bound from the delay, not a measurement); no other link does."""
    res = worker(["lag", str(nranks), str(iters)], f"lag_wg=1:0:{LAG_US}")
    assert res["ok"], res
    d = res["device_s"]
    half = LAG_US * 1e-6 / 2
    assert d["1-0"] >= half and d["0-1"] >= half, d
    assert all(v < half for k, v in d.items() if k not in ("1-0", "0-1")), d
    assert len(d) == nranks * (nranks - 1)


# ---- 3. a late rank -----------------------------------------------------------
LATE_S = 0.2


@pytest.mark.parametrize("check", [True, False])
def test_a_late_rank(check):
    """rank 2 enters LATE_S late: its rx holds the prefill until it calls and
    is complete when its call returns (Fan.late_call); on a star the hub's link
    to leaf 1 ends without waiting for leaf 2"""
    F = mesh(3, 4096)
    try:
        F.checked_call(MESH3, 3, check, "warm-up")
        F.set_tx_seed(1)
        F.late_call(MESH3, 5, check, {2: LATE_S}, ("late rank, mesh", check))
        F.set_tx_seed(2)
        out = F.late_call(STAR, 5, check, {2: LATE_S}, ("late leaf, star", check))
        hub = {l["peer"]: l["device_s"] for l in out[0][1]}
        assert hub[1] < LATE_S / 2 < hub[2], hub
        assert out[1][0].wall_s < LATE_S / 2 and out[1][1][0]["device_s"] < LATE_S / 2, out[1]
    finally:
        F.close()


# ---- 4. across calls ----------------------------------------------------------
@pytest.mark.parametrize("second_ll", [True, False], ids=["ll-ll", "ll-bulk"])
@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("nranks", [2, 3])
def test_rx_read_between_calls(nranks, check, second_ll):
    """tx rewritten between two calls of 3 iterations (call 2's first push
    lands in the other half than call 1's first); the sleeping rank reads its
    whole rx between them while its peers are inside call 2 already; call 2 an
    LL call again, or a bulk fan call on the links the LL call left"""
    between, want = race(nranks, check, second_ll)
    payload.compare(between, want, 0, f"rx of the sleeping rank between the calls ({nranks}, {check}, {second_ll})")


def test_rx_read_between_calls_fails_without_the_handshake():
    """Negative control, MPX_TEST=no_posted in a process of its own.  An LL
    push lands in the receiver's mailbox row and only the receiver's own
    kernel writes its rx, so between two LL calls rx cannot change whatever
    the peers do: the control's second call is the bulk fan call of the
    ll-bulk case above, whose pushes go straight into the sleeper's rx.  With
    the handshake off the racer does not wait for the post the sleeper's next
    call stores after its LL call, and the comparison the positive test makes
    must fail on exactly the racer's new block."""
    res = worker(["no_posted"], "no_posted")
    assert res["mismatch"] and res["early_block"], res


# ---- 5. hand-over ---------------------------------------------------------------
def pair_call(F, mode, n, iters, what, protocol):
    """a checked pair call between ranks 0 (group 1) and 1 on the fan's buffers"""
    def call():
        F.prefill()
        out, errs = {}, {}

        def side(r):
            h = F.host[1 - r]
            try:
                out[r] = F.c.xfer(mode, 1 if r == 0 else 0, r, 1 - r, iters, F.bufs[r][0], F.bufs[r][1], n,
                                  check_payload=True, expect=O.checksum(h[:n]), expect_ack=O.checksum(h[:1]),
                                  timeout_ms=5000)
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,)) for r in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, (what, errs)
        for r in (0, 1):
            m = 1 if (mode == UNIDIR and r == 0) else n
            assert out[r].check_failures == 0 and out[r].check_iters == iters, (what, r)
            assert out[r].protocol == protocol, (what, r, out[r].protocol)
            payload.assert_region(F.c, F.bufs[r][1], 0, F.host[1 - r][:m], what=f"{what}: rx of rank {r}")
            payload.compare(F.c.read(F.bufs[r][0], F.cap), F.host[r], 0, f"{what}: tx of rank {r}")
        return out
    return F.counted({0: [1], 1: [0]}, iters, call)


def test_hand_over_between_protocols_on_the_same_links(monkeypatch):
    """LL fan (odd) -> pair LL ping-pong 8 B -> pair LL unidir 8192 B (its
    message spans both halves; MPX_LL_MAX lifts the one-GPU threshold) -> bulk
    fan -> pair bulk non-blocking -> LL fan: each call finds the row, the
    posted words and the counters as the one before left them"""
    F = mesh(3, 4096)
    try:
        F.checked_call(MESH3, 3, True, "LL fan, odd")
        pair_call(F, PINGPONG, 8, 3, "pair LL ping-pong", 0)
        monkeypatch.setenv("MPX_LL_MAX", "8192")
        pair_call(F, UNIDIR, 8192, 3, "pair LL unidir, both halves", 0)
        monkeypatch.delenv("MPX_LL_MAX")
        F.set_tx_seed(1)
        F.ll = False
        F.checked_call(MESH3, 3, True, "bulk fan")
        pair_call(F, NONBLOCKING, 8192, 5, "pair bulk non-blocking", 1)
        F.set_tx_seed(2)
        F.ll = True
        F.checked_call(MESH3, 4, True, "LL fan again")
        F.set_tx_seed(3)
        F.checked_call(MESH3, 1, False, "LL fan, from an even push number")
        assert {l: F.counters(*l)["tx_seq"] for l in LINKS3} == {(0, 1): 22, (0, 2): 11, (1, 2): 11}
    finally:
        F.close()


# ---- 6. wraps -------------------------------------------------------------------
@pytest.mark.parametrize("P", [pytest.param(P31, id="2pow31"), pytest.param(P32, id="2pow32")])
def test_pushes_across_inside_one_call(P):
    """every link 4 pushes short of P, crossing inside a 9-iteration checked
    call: the tag (31 bits of the push number) and the half (its lowest bit)"""
    F = mesh(3, 4096)
    try:
        for l in LINKS3:
            F.jump(l, P - 4)
        F.checked_call(MESH3, 9, True, ("inside", P))
        assert {l: F.counters(*l)["tx_seq"] for l in LINKS3} == {l: P + 4 for l in LINKS3}
        F.set_tx_seed(1)
        F.checked_call(MESH3, 2, False, ("beyond", P))
    finally:
        F.close()


def test_links_of_one_rank_at_different_points():
    """link (0, 1) near 2^32, link (0, 2) near 2^31, link (1, 2) fresh: one
    launch whose workgroups hold unrelated push numbers"""
    F = mesh(3, 4095)
    try:
        F.jump((0, 1), P32 - 4)
        F.jump((0, 2), P31 - 4)
        F.checked_call(MESH3, 9, True, "mixed points")
        assert {l: F.counters(*l)["tx_seq"] for l in LINKS3} == {(0, 1): P32 + 4, (0, 2): P31 + 4, (1, 2): 9}
    finally:
        F.close()


def test_call_number_and_token_across():
    """calls and tokens Q - 1, Q, Q + 1 of every link and rank: the posted word
    and the sealed completion line; rank 1 enters call Q late, and its rx must
    hold the prefill until then (posted = Q - 1 must not satisfy a wait for Q)"""
    F = mesh(3, 2049)
    try:
        F.advance(LINKS3, calls_by=Q - 2)
        for r in range(3):
            F.advance_token(r, Q - 2)
        for k in range(3):
            if k:
                F.set_tx_seed(k)
            if k == 1:
                F.late_call(MESH3, 3, True, {1: LATE_S}, ("call Q", k))
            else:
                F.checked_call(MESH3, 3, k == 0, ("call number", k))
            for r, p in LINKS3:
                assert F.counters(r, p)["calls"] == F.counters(p, r)["calls"] == Q - 1 + k, (k, r, p)
            assert all(F.counters(r, (r + 1) % 3)["token"] == Q - 1 + k for r in range(3)), k
    finally:
        F.close()


# ---- 7. lost payload ---------------------------------------------------------------
def test_lost_payload_is_caught(monkeypatch):
    """MPX_TEST=skip_push=2: push 2 of every link arrives with its tags and a
    wrong payload (all ones).  Checked, every rank's call returns MPX_ERR_CHECK
    with exactly one failure per link, and the link's digest is that of three
    good blocks and one block of 0xFF: the failure is iteration 2's.  The
    ranks are usable afterwards."""
    n = 4096
    F = mesh(3, n)
    try:
        monkeypatch.setenv("MPX_TEST", "skip_push=2")

        def call():
            out, errs = F.run(MESH3, 4, check=True)
            assert not out and sorted(errs) == [0, 1, 2], (out, errs)
            return errs
        errs = F.counted(MESH3, 4, call)
        lost = O.checksum(b"\xff" * n)
        for r, e in errs.items():
            assert e.status == mpx.ERR_CHECK, (r, e)
            assert e.timing.check_failures == 2 and e.timing.check_iters == 8 and e.timing.recv_done == 8, r
            assert e.timing.protocol == PROTO_FAN_LL, r
            for l in e.links:
                good = O.checksum(F.block(l["peer"], r))
                assert l["check_failures"] == 1 and l["recv_done"] == 4, (r, l)
                assert l["recv_digest"] == (3 * good + lost) & M64, (r, l)
        monkeypatch.setenv("MPX_TEST", "")
        F.set_tx_seed(1)
        F.checked_call(MESH3, 4, True, "after the knob")
    finally:
        F.close()


# ---- 8. refusals ----------------------------------------------------------------
def _status(F, r, peers, block_len=None, stride=None, iters=3, **kw):
    try:
        F.c.fan(r, peers, iters, F.bufs[r][0], F.bufs[r][1], F.block_len if block_len is None else block_len,
                F.stride if stride is None else stride, timeout_ms=2000, **kw)
    except mpx.MpxError as e:
        return e.status
    return mpx.OK


def _raw_status(F, r, peers, flags):
    """mpx_xfer_fan with any flags word"""
    arr = (C.c_int * len(peers))(*peers)
    o = mpx.FanOpts(check=0, flags=flags, timeout_ms=2000, nwg=0, expect_checksum=None)
    t = mpx.Timing()
    return F.c.L.mpx_xfer_fan(F.c.h, r, len(peers), arr, 3, C.c_void_p(F.bufs[r][0].ptr), C.c_void_p(F.bufs[r][1].ptr),
                              F.block_len, F.stride, C.byref(o), C.byref(t), None)


def test_refusals_leave_the_rank_usable(monkeypatch):
    """the four refusals of the flag, each MPX_ERR_INVALID before any GPU work
    (the peers do not call) and without a number taken from the links;
    MPX_FAN_WG does not widen an LL call; a valid call follows"""
    F = LLFan(3, 3 * 8192 + payload.GUARD)
    try:
        F.layout(4096, 8192)
        before = {(r, p): F.counters(r, p) for r in range(3) for p in range(3) if p != r}
        assert mpx.XFER_FAN_LL == 8 and mpx.FAN_LL_MAX == LL_MAX == 4096
        assert _status(F, 0, [1, 2], block_len=4097, ll=True) == mpx.ERR_INVALID      # above the cap
        assert b"MPX_FAN_LL_MAX" in F.c.L.mpx_last_error()
        assert _status(F, 0, [1, 2], block_len=8192, ll=True) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], ll=True, stream=True) == mpx.ERR_INVALID           # with MPX_XFER_STREAM
        assert _status(F, 0, [1, 2], ll=True, nwg=2) == mpx.ERR_INVALID                 # wider than one workgroup
        for extra in (mpx.XFER_PULL, mpx.XFER_NOSTAGE, 16, 1 << 30):                    # any other flag bit
            assert _raw_status(F, 0, [1, 2], mpx.XFER_FAN_LL | extra) == mpx.ERR_INVALID, extra
            assert _raw_status(F, 0, [1, 2], extra) == mpx.ERR_INVALID, extra
        # what the call refused before, it refuses with the flag too
        assert _status(F, 0, [1, 1], ll=True) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], stride=4096 + 8, ll=True) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], stride=16384, ll=True) == mpx.ERR_INVALID          # block 2 past the length
        assert before == {k: F.counters(*k) for k in before}
        monkeypatch.setenv("MPX_FAN_WG", "4")
        F.checked_call(MESH3, 3, True, "after the refusals, MPX_FAN_WG=4", nwg=1)
        monkeypatch.delenv("MPX_FAN_WG")
        F.set_tx_seed(1)
        F.checked_call(MESH3, 0, False, "no iterations: only the token")
    finally:
        F.close()
    S = LLFan(2, 2 * 4096 + payload.GUARD, engine="sdma")
    try:
        S.block_len, S.stride = 4096, 4096
        assert _status(S, 0, [1], ll=True) == mpx.ERR_UNSUPPORTED
    finally:
        S.close()


# ---- 9. the peer never calls -----------------------------------------------------
def test_timeout_when_the_peer_never_calls():
    """rank 0 waits 300 ms for a post that never comes: MPX_ERR_TIMEOUT with
    the LL call's own text, and the rank refuses further calls"""
    F = mesh(2, 4096)
    try:
        out, errs = F.run({0: [1]}, 3, check=True, timeout_ms=300)
        assert 0 in errs and errs[0].status == mpx.ERR_TIMEOUT, (out, errs)
        assert "lock-step LL fan exchange timed out" in str(errs[0]), errs[0]
        out, errs = F.run({0: [1]}, 1, check=False, timeout_ms=300, prefill=False)
        assert errs[0].status == mpx.ERR_STATE
    finally:
        F.close()


# ---- 10. eight ranks x seven links; an odd world -----------------------------------
def test_eight_ranks_seven_links_each():
    F = mesh(8, 4096)
    try:
        F.checked_call(full_mesh(8), 33, True, "8 x 7")
    finally:
        F.close()


def test_five_ranks_on_a_ring():
    """an odd world; every rank lists its two neighbours, the odd ranks in the
    other order; the two blocks of the ranks across stay 0xEE"""
    ring = {r: ([(r + 1) % 5, (r - 1) % 5] if r % 2 else [(r - 1) % 5, (r + 1) % 5]) for r in range(5)}
    F = mesh(5, 4095, 4096)
    try:
        F.checked_call(ring, 33, True, "ring of 5")
        F.set_tx_seed(1)
        F.checked_call(ring, 8, False, "ring of 5, unchecked")
    finally:
        F.close()


# ---- 11. two processes over IPC ----------------------------------------------------
def test_two_processes(tmp_path):
    """a rank per process (tests/fan_ll_worker.py ipc): the LL row and the
    posted word written through IPC-mapped mailboxes; 4095 bytes, checked"""
    procs = [subprocess.Popen([sys.executable, WORKER, "ipc", str(tmp_path), str(p)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for p in (0, 1)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=100)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), outs
    for p in (0, 1):
        x = json.loads(outs[p].strip().splitlines()[-1])
        assert x["rank"] == p and x["rx_ok"] and x["tx_ok"] and x["digest_ok"], x
        assert x["protocol"] == PROTO_FAN_LL and x["nwg"] == 1 and x["launches"] == 1, x
        assert x["check_failures"] == 0 and x["check_iters"] == 5 and x["recv_done"] == 5 and x["bytes"] == 2 * 4095 * 5, x
        assert [(l["peer"], l["nwg"], l["recv_done"], l["check_failures"]) for l in x["links"]] == [(1 - p, 1, 5, 0)], x
        b, a = x["before"], x["after"]
        assert a["tx_seq"] == b["tx_seq"] + 5 and a["rx_seq"] == b["rx_seq"] + 5, x
        assert a["calls"] == b["calls"] + 1 and a["token"] == b["token"] + 1, x


# ---- 12. the host front end: mpx_perf -m 2 ------------------------------------------
@pytest.mark.parametrize("B", [8, 4096])
def test_mpx_perf_m2_threads_mode(tmp_path, B):
    """3 ranks x 2 recorded runs (run 0 is dropped): the records of -m 1, and
    one gpu-*.csv line per link with the LL protocol's name and width 1"""
    from test_gpu_host import run
    args = ["-w", "3", "-m", "2", "-c", "2", "-r", "3", "-i", "5", "-b", str(B), "-f", "@G1", "-n", "1", "-p", "1", "-l", "@LOGS"]
    p, recs, side = run(tmp_path, args, names="vm,runsc,runsc", gpus="0,0,0")
    assert p.returncode == 0, p.stderr[-800:]
    assert "FAN: each of 3 ranks" in p.stderr and "(lock-step LL)" in p.stderr
    assert len(recs) == 3 * 2, recs
    assert sorted((int(f[2]), int(f[10])) for f in recs) == [(r, run_id) for r in range(3) for run_id in (1, 2)]
    for f in recs:
        assert len(f) == 11 and int(f[3]) == 3 and int(f[6]) == 2 and f[4] == f[5] == "127.0.0.1", f
        assert int(f[7]) == B and int(f[8]) == 5, f
    assert len(side) == 2 * 6, side
    for run_id in (1, 2):
        lines = [f for f in side if int(f[17]) == run_id]
        assert sorted((int(f[2]), int(f[6])) for f in lines) == [(r, q) for r in range(3) for q in range(3) if q != r]
    for f in side:
        assert f[3] == "kernel" and f[13] == "fan_ll" and int(f[14]) == 1, f
        assert int(f[8]) == B and int(f[9]) == 5 and int(f[15]) == 5 and int(f[16]) == 0, f
        assert int(f[18]) == 5 and float(f[11]) >= 0, f
        want = O.pattern_checksum(B, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, int(f[6]), int(f[2]), int(f[17])))
        assert int(f[19]) == (5 * want) & M64, f


# ---- 13. seeded free run --------------------------------------------------------------
LL_LENS = [0, 1, 7, 8, 9, 16, 17, 2047, 2048, 2049, 4088, 4095, 4096]
BULK_LENS = [17, 4097, 20001]
PAIR_LENS = [0, 8, 2045, 4097]
ROOM = round16(20001) + 4096
STEPS = 100


def plan(seed, nranks=4, steps=STEPS):
    """LL fan steps over random symmetric peer graphs (random peer order per
    rank, sizes up to 4096, iterations 0 - 9, check on and off), mixed with
    bulk fan steps and checked pair calls on the same links"""
    rng = random.Random(seed)
    out = []
    for k in range(steps):
        key = (seed * 4096 + k + 1) & 0xFFFFFF
        x = rng.random()
        if x < 0.15:
            a, b = sorted(rng.sample(range(nranks), 2))
            out.append(dict(kind="pair", key=key, a=a, b=b, mode=rng.choice([PINGPONG, NONBLOCKING, UNIDIR]),
                            n=rng.choice(PAIR_LENS), iters=rng.randint(1, 9)))
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
        ll = x >= 0.3
        if ll:
            n = rng.choice(LL_LENS) if rng.random() < 0.6 else rng.randint(0, LL_MAX)
            iters = rng.randint(0, 9)
        else:
            n, iters = rng.choice(BULK_LENS), rng.choice([0, 1, 3, 17])
        stride = max(16, round16(n))
        if rng.random() < 0.5:
            stride += 16 * rng.randint(1, (ROOM - stride) // 16)
        out.append(dict(kind="fan", ll=ll, key=key, peers=peers, n=n, stride=stride, iters=iters, check=rng.random() < 0.6))
    return out


def run_rank(F, r, steps, fails, done):
    """rank r's side of the plan, never joining the others: before each call
    rx = 0xEE and tx anew from the step's key (device fills), after it the
    whole rx and tx against host bytes, every reported field, its counters"""
    tx, rx = F.bufs[r]
    others = [p for p in range(F.n) if p != r]
    guard = bytes([payload.GUARD_BYTE])

    def counters():
        return {p: F.c.link_counters(r, p) for p in others}

    def check_counters(before, on, iters):
        for p, a in counters().items():
            b, d = before[p], (iters if p in on else 0)
            assert a["tx_seq"] == b["tx_seq"] + d and a["rx_seq"] == b["rx_seq"] + d, ("push numbers", p, b, a)
            assert a["calls"] == b["calls"] + (1 if p in on and iters > 0 else 0), ("call number", p, b, a)
            assert a["token"] == b["token"] + 1, ("token", p, b, a)

    for k, s in enumerate(steps):
        try:
            if s["kind"] == "pair":
                if r not in (s["a"], s["b"]):
                    continue
                peer, group = (s["b"], 1) if r == s["a"] else (s["a"], 0)
                n, iters, mode = s["n"], s["iters"], s["mode"]
                m = 1 if (mode == UNIDIR and group == 1) else n
                theirs = flat_image(F.cap, peer, s["key"])
                F.c.fill(rx, F.cap, mpx.FILL_BYTE, payload.GUARD_BYTE)
                F.fill_tx(r, s["key"])
                before = counters()
                t = F.c.xfer(mode, group, r, peer, iters, tx, rx, n, check_payload=True, expect=O.checksum(theirs[:n]),
                             expect_ack=O.checksum(theirs[:1]), timeout_ms=5000)
                done.append(r)
                assert t.check_failures == 0 and t.check_iters == iters, t.as_dict()
                payload.compare(F.c.read(rx, F.cap), theirs[:m] + guard * (F.cap - m), 0, f"rx of rank {r}")
                check_counters(before, [peer], iters)
                continue
            peers = s["peers"].get(r)
            if not peers:
                continue
            n, stride, iters, check = s["n"], s["stride"], s["iters"], s["check"]
            blocks = [flat_image(F.cap, p, s["key"])[r * stride:r * stride + n] for p in peers]
            sums = [O.checksum(b) for b in blocks]
            F.c.fill(rx, F.cap, mpx.FILL_BYTE, payload.GUARD_BYTE)
            F.fill_tx(r, s["key"])
            before = counters()
            t, links = F.c.fan(r, peers, iters, tx, rx, n, stride, check_payload=check, expect=sums, timeout_ms=5000,
                               ll=s["ll"])
            done.append(r)
            want = bytearray(guard) * F.cap
            if iters > 0:
                for p, b in zip(peers, blocks):
                    want[p * stride:p * stride + n] = b
            payload.compare(F.c.read(rx, F.cap), bytes(want), 0, f"rx of rank {r}")
            payload.compare(F.c.read(tx, F.cap), flat_image(F.cap, r, s["key"]), 0, f"tx of rank {r}")
            np_ = len(peers)
            assert t.protocol == (PROTO_FAN_LL if s["ll"] else 9) and t.launches == 1, t.as_dict()
            assert t.bytes == 2 * n * iters * np_ and t.recv_done == np_ * iters, t.as_dict()
            assert t.recv_digest == (sum(iters * x for x in sums) & M64 if check else 0), t.as_dict()
            assert t.check_failures == 0 and t.check_iters == (np_ * iters if check else 0), t.as_dict()
            assert [l["peer"] for l in links] == list(peers), links
            for j, l in enumerate(links):
                assert l["recv_done"] == iters and l["check_failures"] == 0 and (l["nwg"] == 1 or not s["ll"]), l
                assert l["recv_digest"] == ((iters * sums[j]) & M64 if check else 0), l
            check_counters(before, peers, iters)
        except (AssertionError, mpx.MpxError) as e:
            fails.append((r, k, {a: b for a, b in s.items() if a != "peers"}, str(e)[:300]))
            if isinstance(e, mpx.MpxError) and e.status == mpx.ERR_TIMEOUT:
                return                      # the rank is broken; its links' state is unknown


@pytest.mark.parametrize("seed", [3, 11])
def test_free_running_ranks_keep_every_payload(seed):
    todo = plan(seed)
    kinds = [(s["kind"], s.get("ll")) for s in todo]
    assert kinds.count(("fan", True)) > 50 and kinds.count(("fan", False)) > 5 and kinds.count(("pair", None)) > 5
    expected = sum(2 if s["kind"] == "pair" else len(s["peers"]) for s in todo)
    F = LLFan(4, 4 * ROOM + payload.GUARD)
    fails, done = [], []
    try:
        th = [threading.Thread(target=run_rank, args=(F, r, todo, fails, done)) for r in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        F.close()
    assert not fails, (len(fails), fails[:4])
    assert len(done) == expected > 2 * STEPS, (len(done), expected)
