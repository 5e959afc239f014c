"""Link counters across their wrap points (-m gpu, MI355X; loopback pairs on
GPU 0).

Every other test starts from a fresh context, so the per-link push numbers
(Rank::tx_seq / rx_seq), the call number (Rank::calls, Mailbox.posted) and the
rank's token never leave their first few thousand values.  A link that runs
for days does: push 2^31 restarts the 31-bit LL tag (ll_tag), 2^32 is where
any 32-bit truncation of a sequence number first shows, and at token 2^32 the
low half of the completion word (fin_word) reads 0 like the cleared line.
mpx_test_advance_link puts a link just short of such a point — every mailbox
compare is "word >= a value derived from the counters" and the mailbox holds
only values of the link's past, so a forward jump of both ranks is a state a
long run reaches — and the calls below run across it.

Every expectation comes from host bytes (hostpairs.run_checked): rx byte for
byte with guards, the host's digest, tx unchanged, every payload checked; and
after every call mpx_link_counters must show what the call added.

"near P": the next push is number P - 4.  No case lets an LL message follow a
larger one by an exact multiple of 2^31 pushes (the documented alias of the LL
zone): a link jumps only before its first LL call.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpx
import oracle_py as O
import payload
from hostpairs import (CREDIT_CAP, CREDIT_N, CREDIT_RING, GUARD, NONBLOCKING, P31, P32, PINGPONG, UNIDIR, HostPairs,
                       checked, counted, jump, received)
from payload import assert_region
from proc import run_bounded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

Q = 1 << 32
BOUNDARIES = [pytest.param(P31, id="2pow31"), pytest.param(P32, id="2pow32")]
MODES = [pytest.param(PINGPONG, id="pingpong"), pytest.param(NONBLOCKING, id="nonblocking"),
         pytest.param(UNIDIR, id="unidir")]
BLOCKING = [pytest.param(PINGPONG, id="pingpong"), pytest.param(UNIDIR, id="unidir")]
PROTO_LL, PROTO_BULK, PROTO_SDMA, PROTO_PULL, PROTO_SDMA_PULL = 0, 1, 2, 7, 8
BULK_NWG, BULK_N = 70, 71681                    # payload.EDGE_CASES: an empty last chunk
HOW = {"push": {}, "push_stream": {"stream": True}, "pull": {"pull": True}}
RESULT_FIELDS = ("recv_done", "recv_digest", "check_iters", "check_failures", "bytes", "protocol", "nwg")


def unchecked(P, mode, n, iters, what, **kw):
    """an unchecked call on a 0xEE-prefilled rx: the reference's receive
    count, then rx byte for byte with its guard and tx unchanged"""
    def call():
        for r in (0, 1):
            P.c.fill(P.bufs[r][1], max(n, 1) + GUARD, mpx.FILL_BYTE, payload.GUARD_BYTE)
        out, errs = P.run(mode, n, iters, check=False, **kw)
        assert not errs, (what, errs)
        done = O.lib().oracle_nb_waited(iters) if mode == NONBLOCKING else iters
        for r in (0, 1):
            assert out[r].recv_done == done, (what, r, out[r].recv_done)
            assert_region(P.c, P.bufs[r][1], 0, P.host[P.peer(r)][:received(mode, r, n)], what=f"{what}: rx of rank {r}")
            payload.compare(P.c.read(P.bufs[r][0], P.cap), P.host[r], 0, f"{what}: tx of rank {r} after the call")
        return out
    return counted(P, iters, call, what)


def protocols(out):
    return [out[r].protocol for r in (0, 1)]


# --------------------------------------------------------------------------
# push numbers: 2^31 (the LL tag restarts) and 2^32
# --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", BLOCKING)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_ll_messages_across(P, mode):
    """LL messages with the boundary inside a call (9 pushes from near P) and
    between two calls (the first ends on push P - 1, the second starts at P).
    At P = 2^31 the tags run 0xffffffff -> 0x80000000 -> 0x80000001, the last
    the tag of push 1; each size has a link of its own, so no unit of the
    landing zone carries an older tag when the link jumps."""
    for n in (0, 1, 8, 2045):
        for calls in ((9,), (4, 4)):
            X = HostPairs(2045 + GUARD)
            try:
                jump(X, P - 4)
                for k, iters in enumerate(calls):
                    out = checked(X, mode, n, iters, ("ll", P, mode, n, calls, k))
                    assert protocols(out) == [PROTO_LL, PROTO_LL]
                    if calls == (4, 4) and k == 0:
                        assert X.counters(0)["tx_seq"] == P - 1
                assert X.counters(0)["tx_seq"] == P - 5 + sum(calls)
            finally:
                X.close()


@pytest.mark.parametrize("mode", BLOCKING)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_ll_zone_history_across(monkeypatch, P, mode):
    """The whole 8 KiB landing zone written just below P, then nine 8-byte
    messages across P (only the first unit is rewritten), then the whole zone
    again: units 1.. still carry the tags of pushes P - 6 and P - 5 and must
    not be taken for the new ones.  tx changes between the calls, so a unit
    accepted with its old tag delivers old bytes."""
    monkeypatch.setenv("MPX_LL_MAX", "8192")
    rng = np.random.default_rng(31)
    X = HostPairs(8192 + GUARD)
    try:
        jump(X, P - 6)
        for n, iters in ((8192, 2), (8, 9), (8192, 3)):
            X.set_tx(rng.integers(0, 256, 8192, dtype=np.uint8).tobytes())
            out = checked(X, mode, n, iters, ("ll zone", P, mode, n))
            assert protocols(out) == [PROTO_LL, PROTO_LL]
        assert X.counters(0)["tx_seq"] == P + 7
    finally:
        X.close()


@pytest.mark.parametrize("how", sorted(HOW))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_bulk_messages_across(P, mode, how):
    """Bulk pushes (plain and streaming stores) and pulls, 70 workgroups with
    an empty last chunk, 9 iterations from near P: the u64 flag, credit,
    ready and landed compares of k_xfer, k_xfer_nbcheck and k_xfer_pull"""
    X = HostPairs(BULK_N + GUARD)
    try:
        jump(X, P - 4)
        out = checked(X, mode, BULK_N, 9, ("bulk", P, mode, how), nwg=BULK_NWG, **HOW[how])
        assert protocols(out) == [PROTO_PULL if how == "pull" else PROTO_BULK] * 2
        assert [out[r].nwg for r in (0, 1)] == [BULK_NWG, BULK_NWG]
    finally:
        X.close()


def test_nonblocking_check_credits_across():
    """Non-blocking check mode with three receive slots per link, 20
    iterations from near 2^31 and near 2^32, pushed and pulled: from the
    fourth push on every push waits for the credit of the push three before
    it (k_xfer_nbcheck).  The ring size is read once per process, so the
    calls run in a child (tests/wrap_worker.py credits)."""
    ring = payload.ring_bytes_for(CREDIT_CAP, CREDIT_RING)
    assert ring == 2 * CREDIT_CAP and payload.ring_slots(ring, CREDIT_N) == 3
    env = dict(os.environ, MPX_CHECK_RING_BYTES=str(CREDIT_RING))
    p = run_bounded([sys.executable, os.path.join(HERE, "wrap_worker.py"), "credits"], env=env, timeout=100)
    assert p.returncode == 0 and p.stdout.split()[-1:] == ["ok"], (p.stdout[-400:], p.stderr[-1200:])


@pytest.mark.parametrize("P", BOUNDARIES)
def test_nonblocking_window_flush_across(P):
    """The kernel engine's unchecked non-blocking loop, 300 one-byte messages
    starting at push P - 250: the Waitall at slot 255 waits for flag >= P + 4
    (wait_bulk(rxs + i)), the final one for P + 49"""
    X = HostPairs(1 + GUARD)
    try:
        jump(X, P - 250)
        out = unchecked(X, NONBLOCKING, 1, 300, ("nb flush", P))
        assert protocols(out) == [PROTO_BULK, PROTO_BULK]
        assert X.counters(0)["tx_seq"] == P + 49
    finally:
        X.close()


SDMA_N, SDMA_ITERS = 65541, 519


SDMA_FORMS = [pytest.param(PINGPONG, False, id="pingpong"), pytest.param(NONBLOCKING, False, id="nonblocking"),
              pytest.param(UNIDIR, False, id="unidir"), pytest.param(PINGPONG, True, id="pingpong-pulled")]


@pytest.mark.parametrize("mode,pull", SDMA_FORMS)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_sdma_graph_chunks_across(P, mode, pull):
    """The SDMA engine's graph-replayed chunks (two of 256 iterations, then 7
    enqueued plainly) with P inside the second chunk: k_signal / k_wait add a
    device-side base that k_seqbase set from the host's counters and advances
    per chunk.  Then a checked call (plain enqueue, absolute values)."""
    X = HostPairs(SDMA_N + GUARD, engine="sdma")
    try:
        jump(X, P - 356)                      # chunk 2 is pushes P - 100 .. P + 155
        out = unchecked(X, mode, SDMA_N, SDMA_ITERS, ("sdma chunks", P, mode, pull), pull=pull)
        assert protocols(out) == [PROTO_SDMA_PULL if pull else PROTO_SDMA] * 2
        assert X.counters(0)["tx_seq"] == P + 162
        checked(X, mode, SDMA_N, 5, ("sdma checked after chunks", P, mode, pull), pull=pull)
    finally:
        X.close()


@pytest.mark.parametrize("mode,pull", SDMA_FORMS)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_sdma_checked_calls_across(P, mode, pull):
    """The unchecked loop above re-sends the same bytes, so a k_wait that lets
    a stream run ahead leaves the same final rx.  A checked call of 9
    iterations from near P (plain enqueue: flag, credit and ready values
    absolute) checksums and poisons every receive on the stream right behind
    its wait: a wait that passes early checksums the poison."""
    X = HostPairs(SDMA_N + GUARD, engine="sdma")
    try:
        jump(X, P - 4)
        out = checked(X, mode, SDMA_N, 9, ("sdma checked", P, mode, pull), pull=pull)
        assert protocols(out) == [PROTO_SDMA_PULL if pull else PROTO_SDMA] * 2
    finally:
        X.close()


B_LL, B_BULK = 8, 65536 + 13


@pytest.mark.parametrize("kind", ["ll", "bulk", "pull"])
@pytest.mark.parametrize("P", BOUNDARIES)
def test_traced_kernels_across(P, kind):
    """The recorder's kernels (k_xfer_lat, k_xfer_pull_lat) across P: what the
    untraced call returns, one recorded iteration per iteration"""
    mode, n, kw = {"ll": (PINGPONG, B_LL, {}), "bulk": (UNIDIR, B_BULK, {}), "pull": (PINGPONG, B_BULK, {"pull": True})}[kind]
    X = HostPairs(B_BULK + GUARD)
    try:
        jump(X, P - 4)
        for r in (0, 1):
            X.c.lat_enable(r, 16)
        out = checked(X, mode, n, 9, ("traced", P, kind), **kw)
        for r in (0, 1):
            lat = X.c.lat_get(r)
            assert lat["count"] == 9 and lat["calls"] == 1 and len(X.c.lat_raw(r)) == 10, (r, lat["count"])
            X.c.lat_disable(r)
        plain = checked(X, mode, n, 9, ("untraced", P, kind), **kw)
        for r in (0, 1):
            assert {f: getattr(out[r], f) for f in RESULT_FIELDS} == {f: getattr(plain[r], f) for f in RESULT_FIELDS}
        assert protocols(out) == [{"ll": PROTO_LL, "bulk": PROTO_BULK, "pull": PROTO_PULL}[kind]] * 2
    finally:
        X.close()


# --------------------------------------------------------------------------
# call numbers and tokens: Q = 2^32
# --------------------------------------------------------------------------
def near_q(X, next_number=Q - 2):
    """the link's next call and the ranks' next token are `next_number`"""
    c = X.counters(0)
    assert c == X.counters(1)
    X.advance(calls_by=next_number - 1 - c["calls"], token_by=next_number - 1 - c["token"])


def phases_are_real(X, what):
    for r in (0, 1):
        ph = X.c.phases(r)
        assert ph["kernel_s"] > 0 and ph["wall_s"] >= ph["kernel_s"], (what, r, ph)


def test_five_calls_across_the_token_wrap():
    """Calls Q - 2 .. Q + 2 of a link, tokens alike: the third call's token
    has a low word of 0, the value of the cleared completion line.  It must
    complete on the kernel's sealed line, not on the cleared one: receive
    count, digest and bytes are the call's, and its phases are non-zero."""
    X = HostPairs(BULK_N + GUARD)
    try:
        near_q(X)
        plan = [("ll", PINGPONG, 2045, {}), ("bulk", PINGPONG, BULK_N, {"nwg": BULK_NWG}),
                ("pulled", PINGPONG, BULK_N, {"nwg": BULK_NWG, "pull": True}),
                ("nonblocking checked", NONBLOCKING, BULK_N, {"nwg": BULK_NWG}), ("unidir", UNIDIR, BULK_N, {"nwg": BULK_NWG})]
        for k, (name, mode, n, kw) in enumerate(plan):
            checked(X, mode, n, 9, (name, "call", Q - 2 + k), **kw)
            for r in (0, 1):
                c = X.counters(r)
                assert c["token"] == c["calls"] == Q - 2 + k, (name, r, c)
            phases_are_real(X, name)
    finally:
        X.close()


def test_armed_calls_across_the_token_wrap():
    """go_token, Status.ready and the completion word of armed calls at
    tokens Q - 2, Q - 1 and Q; then both sides armed at token 2Q (low word 0
    again) and disarmed — the token is spent, the call number and the push
    numbers are not — and a checked call after it"""
    X = HostPairs(BULK_N + GUARD)
    try:
        near_q(X)
        for k, (mode, n) in enumerate([(PINGPONG, 2045), (UNIDIR, BULK_N), (PINGPONG, BULK_N)]):
            checked(X, mode, n, 9, ("armed", Q - 2 + k), armed=True)
            assert X.counters(0)["token"] == Q - 2 + k
            phases_are_real(X, ("armed", k))
            assert all(X.c.phases(r)["armed"] == 1 for r in (0, 1))
        X.advance(token_by=2 * Q - 1 - X.counters(0)["token"])
        before = [X.counters(r) for r in (0, 1)]
        for r in (0, 1):
            exp = X.expect(r, BULK_N)
            X.c.arm(PINGPONG, X.group(r), r, X.peer(r), 9, X.bufs[r][0], X.bufs[r][1], BULK_N, check_payload=True,
                    expect=exp[0], expect_ack=exp[1], timeout_ms=10000)
            # an armed rank's counters stay where they are
            with pytest.raises(mpx.MpxError) as e:
                X.c.test_advance_link(r, X.peer(r), 1, 0, 0)
            assert e.value.status == mpx.ERR_STATE
        for r in (0, 1):
            X.c.disarm(r)
        for r in (0, 1):
            a = X.counters(r)
            assert a["token"] == before[r]["token"] + 1 == 2 * Q, (r, before[r], a)
            assert {k: a[k] for k in ("tx_seq", "rx_seq", "calls")} == {k: before[r][k] for k in ("tx_seq", "rx_seq", "calls")}
        checked(X, PINGPONG, BULK_N, 9, "after the disarm")
    finally:
        X.close()


def test_failed_launch_gives_every_counter_back(monkeypatch):
    """MPX_TEST=fail_launch=0 with rank 0's next token Q - 1, armed and
    unarmed: give_back gives the token and the call number back, so
    every counter is where it was; the next calls (tokens Q - 1 and Q) pass"""
    X = HostPairs(BULK_N + GUARD)
    try:
        near_q(X, Q - 1)
        before = X.counters(0)
        assert before["token"] == before["calls"] == Q - 2
        monkeypatch.setenv("MPX_TEST", "fail_launch=0")
        args = (PINGPONG, X.group(0), 0, 1, 9, X.bufs[0][0], X.bufs[0][1], BULK_N)
        for call in (X.c.arm, X.c.xfer):
            with pytest.raises(mpx.MpxError) as e:
                call(*args)
            assert "fail_launch" in str(e.value)
            assert X.counters(0) == before
        monkeypatch.setenv("MPX_TEST", "")
        for k in (0, 1):
            checked(X, PINGPONG, BULK_N, 9, ("after the failed launches", k))
            assert X.counters(0)["token"] == Q - 1 + k
    finally:
        X.close()


def test_sdma_posted_handshake_across_the_call_wrap():
    """The SDMA engine's receive-posted handshake (signal_abs / wait_abs of
    Rank::calls) at calls Q - 2 .. Q + 2; the engine has no token"""
    X = HostPairs(4097 + GUARD, engine="sdma")
    try:
        near_q(X)
        plan = [(PINGPONG, {}), (UNIDIR, {}), (NONBLOCKING, {}), (PINGPONG, {"pull": True}), (UNIDIR, {})]
        for k, (mode, kw) in enumerate(plan):
            checked(X, mode, 4097, 5, ("sdma call", Q - 2 + k, mode), **kw)
            assert X.counters(0)["calls"] == X.counters(1)["calls"] == Q - 2 + k
    finally:
        X.close()


# --------------------------------------------------------------------------
# two processes, a detected loss, the mover's contract
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n,protocol", [pytest.param(8, PROTO_LL, id="ll"), pytest.param(65541, PROTO_BULK, id="bulk")])
def test_two_processes_across_the_tag_wrap(tmp_path, n, protocol):
    """Each process advances its own side right after attach and import
    (tests/ipc_worker.py), then a 9-iteration call across 2^31 through the
    IPC-mapped mailbox and rx, and a unidir call after it"""
    cmd = [sys.executable, os.path.join(HERE, "ipc_worker.py"), str(tmp_path)]
    procs = [subprocess.Popen(cmd + [str(r), "kernel", "same", str(P31 - 5), str(n)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in (0, 1)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=100)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), outs
    for r in (0, 1):
        res = json.load(open(tmp_path / f"result_{r}.json"))
        assert [x["mode"] for x in res] == [PINGPONG, UNIDIR]
        last = P31 - 5
        for x in res:
            assert x["final_rx_ok"] and x["check_failures"] == 0 and x["check_iters"] == x["iters"] == 9, (r, x)
            assert x["recv_done"] == 9 and x["protocol"] == protocol, (r, x)
            assert x["before"]["tx_seq"] == x["before"]["rx_seq"] == last, (r, x)
            last += 9
            assert x["after"]["tx_seq"] == x["after"]["rx_seq"] == last, (r, x)
            assert x["after"]["calls"] == x["before"]["calls"] + 1 and x["after"]["token"] == x["before"]["token"] + 1
            # the imported rank's counters live in its own process
            assert x["imported_rank_status"] == mpx.ERR_INVALID, (r, x)


@pytest.mark.parametrize("P", BOUNDARIES)
def test_counters_after_a_detected_loss(monkeypatch, P):
    """MPX_TEST=skip_push=2 on a checked 5-iteration bulk call across P: both
    ping-pong receivers report MPX_ERR_CHECK.  The loop itself completed —
    every flag went — so complete_call has counted its pushes before
    finish_xfer (mpx_xfer_ex) compares the checksums: the counters stand
    where a passing call leaves them, and the next checked call passes."""
    X = HostPairs(BULK_N + GUARD)
    try:
        jump(X, P - 4)

        def lossy():
            out, errs = X.run(PINGPONG, BULK_N, 5, nwg=BULK_NWG)
            assert sorted(errs) == [0, 1] and not out, (out, errs)
            assert all(errs[r].status == mpx.ERR_CHECK for r in (0, 1)), errs
            assert all("1 of 5 received payloads" in str(errs[r]) for r in (0, 1)), errs

        monkeypatch.setenv("MPX_TEST", "skip_push=2")
        counted(X, 5, lossy, ("lossy", P))
        monkeypatch.setenv("MPX_TEST", "")
        assert X.counters(0)["tx_seq"] == P
        checked(X, PINGPONG, BULK_N, 5, ("after the loss", P), nwg=BULK_NWG)
    finally:
        X.close()


def test_the_mover_is_refused_without_the_test_gate():
    """A process started without MPX_TEST (bench.py, mpx_perf): the mover
    returns MPX_ERR_UNSUPPORTED, the getter works (tests/wrap_worker.py)"""
    env = {k: v for k, v in os.environ.items() if k != "MPX_TEST"}
    p = run_bounded([sys.executable, os.path.join(HERE, "wrap_worker.py"), "nogate"], env=env, timeout=100)
    assert p.returncode == 0 and p.stdout.split()[-1:] == ["ok"], (p.stdout[-400:], p.stderr[-1200:])


def test_the_movers_arguments():
    X = HostPairs(64 + GUARD)
    try:
        L, h = X.c.L, X.c.h
        out = (ctypes.c_uint64 * 4)()
        assert L.mpx_link_counters(None, 0, 1, out) == mpx.ERR_INVALID
        assert L.mpx_link_counters(h, 0, 1, None) == mpx.ERR_INVALID
        for my, peer in ((-1, 0), (2, 0), (0, -1), (0, 2)):
            assert L.mpx_link_counters(h, my, peer, out) == mpx.ERR_INVALID, (my, peer)
            assert L.mpx_test_advance_link(h, my, peer, 1, 1, 1) == mpx.ERR_INVALID, (my, peer)
        assert L.mpx_test_advance_link(None, 0, 1, 1, 1, 1) == mpx.ERR_INVALID
        # it adds, per link and per rank, and never passes 2^64
        X.c.test_advance_link(0, 1, 5, 3, 2)
        assert X.counters(0) == dict(tx_seq=5, rx_seq=5, calls=3, token=2)
        assert X.counters(1) == dict(tx_seq=0, rx_seq=0, calls=0, token=0)
        assert X.c.link_counters(0, 0) == dict(tx_seq=0, rx_seq=0, calls=0, token=2)
        X.c.test_advance_link(0, 1, 0, 0, 0)
        for by in ((2**64 - 5, 0, 0), (0, 2**64 - 3, 0), (0, 0, 2**64 - 2)):
            assert L.mpx_test_advance_link(h, 0, 1, *by) == mpx.ERR_INVALID, by
        assert X.counters(0) == dict(tx_seq=5, rx_seq=5, calls=3, token=2)
        X.c.test_advance_link(1, 0, 5, 3, 2)
        checked(X, PINGPONG, 64, 3, "after advancing both sides")
    finally:
        X.close()
