"""Fan links across their counters' wrap points (-m gpu, MI355X; loopback
ranks on GPU 0, tests/fan.py).

tests/test_gpu_wrap.py runs the pair loops across push 2^31 / 2^32 and call /
token 2^32.  k_xfer_fan shares none of their waits: it has a wait_ge of its
own, its push and call numbers travel through a table of its own (FanLink
tx_seq0 / rx_seq0 / call, written by the host into a pinned image and copied
to the device), and its posted / flag / credit values are derived from that
table.  A 32-bit cut anywhere on that path shows first at 2^32 (low word 0,
smaller than the word the mailbox still holds), so every case here puts a
link just short of such a point (mpx_test_advance_link, both sides alike) and
runs across it.

Every expectation is host bytes (Fan.verify: rx whole against the peers'
blocks and 0xEE, tx whole, host digests, every reported field) and after
every call every link's counters are read back from both sides
(Fan.counted).  "near P": the next push is number P - 4.  mesh3, 65555 bytes
(5 workgroups per link, a ragged tail) unless stated.  No case may time out:
every deadline is 5000 ms and none is expected to be used.
"""
import json
import os
import subprocess
import sys
import threading

import pytest

import mpx
import oracle_py as O
import payload
from fan import Fan, full_mesh, round16
from payload import chunk_shape

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

P31, P32 = 1 << 31, 1 << 32
Q = 1 << 32
BOUNDARIES = [pytest.param(P31, id="2pow31"), pytest.param(P32, id="2pow32")]
PINGPONG, NONBLOCKING = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING
N = 65555
MESH3 = full_mesh(3)
LINKS3 = [(0, 1), (0, 2), (1, 2)]
EDGE_NWG, EDGE_N = 96, 98305          # tests/test_gpu_fan.py: chunks of 1040 B, one empty, one of 545 B


def mesh3(n=N):
    F = Fan(3, 3 * round16(n) + payload.GUARD)
    F.layout(n, round16(n))
    return F


def tx_seqs(F):
    return {l: F.counters(*l)["tx_seq"] for l in LINKS3}


# (check, stream, iters, back): the call starts at push P - back.  Without
# check mode a flag goes every 16 pushes and at the last: 17 pushes from
# P - 4 publish P + 11 and P + 12; 33 pushes from P - 20 publish P - 5, P + 11
# and P + 12, a mid-loop flag on either side of P.
INSIDE = [pytest.param(True, False, 9, 4, id="check"), pytest.param(True, True, 9, 4, id="check-stream"),
          pytest.param(False, False, 9, 4, id="plain-9"), pytest.param(False, False, 17, 4, id="plain-17"),
          pytest.param(False, False, 33, 20, id="plain-33")]


@pytest.mark.parametrize("check,stream,iters,back", INSIDE)
@pytest.mark.parametrize("P", BOUNDARIES)
def test_pushes_across_inside_one_call(P, check, stream, iters, back):
    """every link of the mesh crosses P inside one call: the flag, credit and
    last-flag compares of k_xfer_fan on numbers either side of P"""
    F = mesh3()
    try:
        for l in LINKS3:
            F.jump(l, P - back)
        F.checked_call(MESH3, iters, check, ("inside", P, check, stream, iters), widths=5, stream=stream)
        assert tx_seqs(F) == {l: P - back - 1 + iters for l in LINKS3}
        assert P - back - 1 + iters > P
    finally:
        F.close()


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("P", BOUNDARIES)
def test_chunk_edges_across(P, check):
    """explicit width 96 at 98305 bytes: the empty workgroup and the one with
    545 bytes publish, credit and count across P like every other"""
    assert chunk_shape(EDGE_NWG, EDGE_N) == (96, 1040, 1, 94, 545)
    F = mesh3(EDGE_N)
    try:
        for l in LINKS3:
            F.jump(l, P - 4)
        F.checked_call(MESH3, 9, check, ("edges", P, check), widths=EDGE_NWG, nwg=EDGE_NWG)
        assert tx_seqs(F) == {l: P + 4 for l in LINKS3}
    finally:
        F.close()


LATE_S = 0.2


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("P", BOUNDARIES)
def test_boundary_between_two_calls(P, check):
    """the first call ends on push P - 1 and is call 2^32 - 1 of every link, the
    second starts at push P and is call 2^32: tx_seq0 = P - 1 and the call
    number go through the table, and at P = 2^32 every mailbox word the second
    call waits on (posted, flag, credit) still holds a value whose low half
    is 0xffffffff while the call asks for low halves 0 .. 3.  Rank 2 enters
    the second call LATE_S late: a wait that compared low halves would pass
    at once, so ranks 0 and 1 would push into rank 2's rx before its post and
    return with nothing received from it (Fan.late_call reads rx at both
    moments).  tx is drawn anew between the calls, so a second call that
    moved nothing leaves call 1's bytes and fails the comparison."""
    F = mesh3()
    try:
        for l in LINKS3:
            F.jump(l, P - 4)
        F.advance(LINKS3, calls_by=Q - 2)
        F.checked_call(MESH3, 4, check, ("two calls, first", P, check), widths=5)
        assert tx_seqs(F) == {l: P - 1 for l in LINKS3}
        assert all(F.counters(*l)["calls"] == Q - 1 for l in LINKS3)
        F.set_tx_seed(1)
        F.late_call(MESH3, 4, check, {2: LATE_S}, ("two calls, second", P, check), widths=5)
        assert tx_seqs(F) == {l: P + 3 for l in LINKS3}
        assert all(F.counters(*l)["calls"] == Q for l in LINKS3)
    finally:
        F.close()


@pytest.mark.parametrize("check", [True, False])
def test_links_of_one_rank_at_different_points(check):
    """link (0, 1) near 2^32, link (0, 2) near 2^31, link (1, 2) fresh: every
    rank's table holds unrelated tx_seq0 values in one launch"""
    F = mesh3()
    try:
        F.jump((0, 1), P32 - 4)
        F.jump((0, 2), P31 - 4)
        F.checked_call(MESH3, 9, check, ("mixed points", check), widths=5)
        assert tx_seqs(F) == {(0, 1): P32 + 4, (0, 2): P31 + 4, (1, 2): 9}
        F.set_tx_seed(2)
        F.checked_call(MESH3, 9, not check, ("mixed points, again", check), widths=5)
    finally:
        F.close()


def phases_are_real(F, ranks, what):
    for r in ranks:
        ph = F.c.phases(r)
        assert ph["kernel_s"] > 0 and ph["wall_s"] >= 0.98 * ph["kernel_s"], (what, r, ph)


@pytest.mark.parametrize("check", [True, False])
def test_call_number_across(check):
    """calls Q - 2 .. Q + 1 of every link (the posted word: FanLink.call through
    the table, wait_ge on it), with a call of no iterations in the middle,
    which takes no number and posts the link's last one again.  Rank 1 enters
    call Q late: its rx must hold the prefill until it calls (posted = Q - 1,
    low half 0xffffffff, must not satisfy a wait for Q), and nobody is done
    before it has called."""
    F = mesh3()
    try:
        F.advance(LINKS3, calls_by=Q - 3)
        number = Q - 3
        for k, (iters, chk) in enumerate([(3, check), (3, not check), (0, True), (3, check), (3, not check)]):
            F.set_tx_seed(10 + k)
            if iters and number + 1 == Q:
                F.late_call(MESH3, iters, chk, {1: LATE_S}, ("call number Q", chk), widths=5)
            else:
                F.checked_call(MESH3, iters, chk, ("call number", k, chk), widths=5)
            number += 1 if iters else 0
            for r, p in LINKS3:
                assert F.counters(r, p)["calls"] == F.counters(p, r)["calls"] == number, (k, r, p)
        assert number == Q + 1
    finally:
        F.close()


def test_token_across():
    """every rank's tokens Q - 2 .. Q + 1: the third call's completion word has
    a low half of 0, the value of the cleared line; the call must complete on
    the kernel's sealed line (its counts, digests, bytes and non-zero phases)"""
    F = mesh3()
    try:
        for r in range(3):
            F.advance_token(r, Q - 3)
        for k, (iters, check) in enumerate([(3, True), (3, False), (3, True), (0, False)]):
            F.set_tx_seed(20 + k)
            F.checked_call(MESH3, iters, check, ("token", k), widths=5)
            for r in range(3):
                assert F.counters(r, (r + 1) % 3)["token"] == Q - 2 + k, (k, r)
            phases_are_real(F, range(3), ("token", k))
    finally:
        F.close()


def pair_call(F, mode, n, iters, what):
    """a checked pair call between ranks 0 and 1 on the fan's buffers (the
    first n bytes of tx and rx), from host bytes, with the link's counters"""
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
            assert out[r].check_failures == 0 and out[r].check_iters == iters, (what, r)
            payload.assert_region(F.c, F.bufs[r][1], 0, F.host[1 - r][:n], what=f"{what}: rx of rank {r}")
            payload.compare(F.c.read(F.bufs[r][0], F.cap), F.host[r], 0, f"{what}: tx of rank {r}")
        return out
    return F.counted({0: [1], 1: [0]}, iters, call)


@pytest.mark.parametrize("P", BOUNDARIES)
def test_fan_crosses_then_pair_calls(P):
    """a fan call takes the links across P; a checked bulk ping-pong, a checked
    non-blocking call and an 8-byte LL call then run on link (0, 1) from the
    counters and mailbox words the fan call left, and a fan call after them"""
    F = mesh3()
    try:
        for l in LINKS3:
            F.jump(l, P - 4)
        F.checked_call(MESH3, 9, True, ("fan across", P), widths=5)
        out = pair_call(F, PINGPONG, N, 5, ("ping-pong after the fan", P))
        assert [out[r].protocol for r in (0, 1)] == [1, 1]
        pair_call(F, NONBLOCKING, N, 5, ("non-blocking after the fan", P))
        out = pair_call(F, PINGPONG, 8, 3, ("LL after the fan", P))       # the link's first LL call
        assert [out[r].protocol for r in (0, 1)] == [0, 0]
        F.set_tx_seed(3)
        F.checked_call(MESH3, 3, False, ("fan after the pair calls", P), widths=5)
        assert tx_seqs(F) == {(0, 1): P + 20, (0, 2): P + 7, (1, 2): P + 7}
    finally:
        F.close()


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("P", BOUNDARIES)
def test_pair_call_crosses_then_fan(P, check):
    """the other order: a checked ping-pong takes link (0, 1) across P, a
    non-blocking one follows, then fan calls on the mesh (its other two links
    fresh) read the link's numbers where the pair calls left them"""
    F = mesh3()
    try:
        F.jump((0, 1), P - 4)
        pair_call(F, PINGPONG, N, 9, ("ping-pong across", P))
        pair_call(F, NONBLOCKING, N, 5, ("non-blocking beyond", P))
        F.checked_call(MESH3, 9, check, ("fan after the pair calls", P, check), widths=5)
        F.set_tx_seed(4)
        F.checked_call(MESH3, 17, not check, ("fan again", P, check), widths=5)
        assert tx_seqs(F) == {(0, 1): P + 35, (0, 2): 26, (1, 2): 26}
    finally:
        F.close()


def test_two_processes_across(tmp_path):
    """two processes with two ranks each (tests/fan_worker.py jump=2^32 - 1):
    each advances its own side of its ranks' links, so push 2 of 3 is number
    2^32 on all three links of every rank, two of them over imported ranks
    (IPC-mapped mailbox and rx)"""
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fan_worker.py"), str(tmp_path), str(p),
                               f"jump={P32 - 1}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for p in (0, 1)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=100)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), outs
    for p in (0, 1):
        res = json.load(open(tmp_path / f"result_{p}.json"))
        assert sorted(x["rank"] for x in res) == [2 * p, 2 * p + 1]
        for x in res:
            assert x["rx_ok"] and x["tx_ok"] and x["digest_ok"] and x["protocol"] == 9, x
            assert x["check_failures"] == 0 and x["check_iters"] == 9 and x["recv_done"] == 9 and x["iters"] == 3, x
            assert [l["recv_done"] for l in x["links"]] == [3] * 3, x
            for b, a in zip(x["before"], x["after"]):
                assert b["tx_seq"] == b["rx_seq"] == P32 - 2, x
                assert a["tx_seq"] == a["rx_seq"] == P32 + 1, x
                assert a["calls"] == b["calls"] + 1 and a["token"] == b["token"] + 1, x
