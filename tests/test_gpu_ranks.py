"""Rank numbers 8 to 63, and links whose two ends differ (-m gpu).

Every table the library indexes by rank has 64 rows (MPX_MAX_RANKS): the
mailbox's flag / ll / credit / posted / ready rows, a rank's tx_seq / rx_seq /
calls, the fan table and FanLink.off = peer * stride, RankDesc.rank.  Here a
64-rank context has two to six ranks attached, with numbers that collide
modulo 8, 16 and 32 (5, 13, 21, 37; 62, 63; 9, 1, 40), so an index that lost
its high bits would alias two live rows.  The links stand at distinct counts
(mpx_test_advance_link), calls of different sizes, modes and protocols run on
them at once, and after every round tests/links.py compares the whole of every
attached rank's rx and tx with host bytes and every counter row with what the
round must have added: rows of links that did not call are unchanged.

The second half: links whose ends were attached with different lengths
(4097 + GUARD bytes and 1 MiB), and pairs whose higher rank number is group 1.
"""
import json
import os
import subprocess
import sys

import pytest

import fan as F
import mpx
import oracle_py as O
from hostpairs import CREDIT_CAP, CREDIT_N, CREDIT_RING, GUARD
from links import (NONBLOCKING, PINGPONG, PROTO_BULK, PROTO_LL, PROTO_PULL, PROTO_SDMA, PROTO_SDMA_PULL, UNIDIR, Links,
                   link)
from proc import run_bounded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

BULK_N = 65541          # bulk push; at the explicit width 7 (chunks of 9376 B, the last one 9285)
CAP = BULK_N + GUARD
RANKS = [5, 13, 21, 37, 62, 63]


def spread(X):
    """the links at distinct counts, as long runs would have left them"""
    for k, (a, b) in enumerate([(5, 13), (5, 21), (5, 37), (5, 63), (62, 63), (21, 37), (13, 37), (13, 21), (62, 13),
                                (63, 63)]):
        X.advance(a, b, seq_by=1000 * (k + 1), calls_by=3 * k)


def test_sparse_ranks_kernel_engine_every_protocol(monkeypatch):
    """Every protocol of the kernel engine on rows 5 to 63, three links at a
    time.  What this can see: a row that does not exist or overlaps its
    neighbour (ranks 62 and 63 are in flight together), a host table indexed
    wrongly (every counter row is compared), bytes at the wrong place.  A
    mailbox row index that merely lost its high bits on both sides alike
    passes here, the links being used at rising counts (hand control: slots
    cut to 3 bits, passed); test_one_receiver_after_senders_that_would_alias
    is the test for that."""
    X = Links("kernel", RANKS, CAP)
    try:
        spread(X)
        X.round([link(5, 13, PINGPONG, 8, 40, proto=PROTO_LL),
                 link(21, 37, UNIDIR, BULK_N, 5, proto=PROTO_BULK, nwg=7),
                 link(62, 63, NONBLOCKING, 4097, 300, proto=PROTO_BULK)], "round 1")
        X.round([link(5, 21, UNIDIR, 2045, 9, proto=PROTO_LL),
                 link(63, 62, PINGPONG, BULK_N, 5, proto=PROTO_BULK, nwg=7, stream=True),    # the higher rank group 1
                 link(37, 13, NONBLOCKING, 8, 300, proto=PROTO_BULK)], "round 2")
        X.round([link(5, 37, PINGPONG, BULK_N, 5, proto=PROTO_PULL, nwg=7, pull=True),
                 link(13, 21, UNIDIR, 8, 40, proto=PROTO_LL),
                 link(63, 63, NONBLOCKING, 4097, 20)], "round 3: pull, LL, rank 63 with itself")
        X.round([link(63, 5, UNIDIR, BULK_N, 5, check=False, proto=PROTO_BULK, nwg=7),
                 link(62, 13, PINGPONG, 2045, 9, check=False, proto=PROTO_LL),
                 link(37, 21, NONBLOCKING, BULK_N, 20, proto=PROTO_PULL, nwg=7, pull=True)], "round 4: unchecked")
        X.round([link(5, 13, PINGPONG, BULK_N, 5, proto=PROTO_BULK, nwg=7, armed=True),
                 link(62, 63, UNIDIR, 2045, 9, proto=PROTO_LL, armed=True),
                 link(21, 37, PINGPONG, 2045, 9, proto=PROTO_LL)], "round 5: armed")
        assert [X.c.phases(r)["armed"] for r in (5, 13, 62, 63, 21, 37)] == [1, 1, 1, 1, 0, 0]
        # a traced call on rank 63 (mpx_lat_enable): its recorder, not rank 5's
        X.c.lat_enable(63, 64)
        X.round([link(5, 63, PINGPONG, 8, 40, proto=PROTO_LL), link(13, 21, UNIDIR, BULK_N, 5, nwg=7)],
                "round 6: traced")
        lat, raw = X.c.lat_get(63), X.c.lat_raw(63)
        assert lat["count"] == 40 and lat["calls"] == 1 and lat["last_iters"] == 40 and len(raw) == 41
        assert all(b >= a for a, b in zip(raw, raw[1:]))
        X.c.lat_disable(63)
        # the LL landing zone's last granules (8185 B = 2047 granules) under the cross-GPU threshold
        monkeypatch.setenv("MPX_LL_MAX", "8192")
        X.round([link(5, 63, PINGPONG, 8185, 9, proto=PROTO_LL),
                 link(37, 21, UNIDIR, 8185, 9, proto=PROTO_LL),
                 link(62, 13, PINGPONG, 8, 9, proto=PROTO_LL)], "round 7: MPX_LL_MAX=8192")
        monkeypatch.delenv("MPX_LL_MAX")
        X.round([link(63, 5, PINGPONG, 2045, 9, proto=PROTO_LL),
                 link(21, 13, UNIDIR, BULK_N, 5, proto=PROTO_BULK, nwg=7, stream=True),
                 link(62, 37, NONBLOCKING, 4097, 300, proto=PROTO_BULK)], "round 8")
    finally:
        X.close()


def test_sparse_ranks_sdma_engine():
    n = 4097
    X = Links("sdma", [5, 13, 37, 63], n + GUARD)
    try:
        spread_sdma = [(5, 13), (37, 63), (5, 37), (13, 63), (5, 63), (13, 37), (63, 63)]
        for k, (a, b) in enumerate(spread_sdma):
            X.advance(a, b, seq_by=1000 * (k + 1), calls_by=3 * k)
        X.round([link(5, 13, PINGPONG, n, 9, proto=PROTO_SDMA), link(37, 63, UNIDIR, 8, 9, proto=PROTO_SDMA)], "push")
        X.round([link(5, 37, NONBLOCKING, n, 300, proto=PROTO_SDMA_PULL, pull=True),
                 link(63, 13, PINGPONG, n, 9, proto=PROTO_SDMA_PULL, pull=True)], "pull")
        # graph chunks: 300 iterations unchecked, then a checked call on the same links
        X.round([link(5, 63, PINGPONG, n, 300, check=False, proto=PROTO_SDMA),
                 link(13, 37, UNIDIR, n, 300, check=False, proto=PROTO_SDMA)], "graph chunks")
        X.round([link(5, 63, PINGPONG, n, 9, proto=PROTO_SDMA), link(13, 37, UNIDIR, n, 9, proto=PROTO_SDMA)],
                "checked after graph chunks")
        X.round([link(63, 63, NONBLOCKING, n, 20, proto=PROTO_SDMA),
                 link(37, 5, NONBLOCKING, n, 300, proto=PROTO_SDMA)],
                "rank 63 with itself, non-blocking check")
    finally:
        X.close()


SENDERS = [37, 21, 13, 5]      # all of them 5 modulo 8; 37, 21 and 5 modulo 16; 37 and 5 modulo 32


@pytest.mark.parametrize("engine", ["kernel", "sdma"])
def test_one_receiver_after_senders_that_would_alias(engine):
    """A rank is in one pair call at a time, so two senders never write one
    receiver's mailbox at once: a row index that lost its high bits shows
    only through what the earlier sender LEFT in the shared row.  The waits
    on flag, ready, credit and posted words are "word >= expected", so the
    links to rank 63 stand at descending counts in the order they are used
    (a stale, higher word lets the receiver go on before its bytes landed);
    the LL wait wants its tag exactly, so each LL link is moved to where its
    first message has the number of the previous link's last."""
    X = Links(engine, SENDERS + [63], CAP)
    try:
        for k, s in enumerate(SENDERS):
            X.advance(s, 63, seq_by=10000 * (4 - k), calls_by=100 * (4 - k))
        for kw in (dict(), dict(pull=True)):
            for mode in (PINGPONG, UNIDIR, NONBLOCKING):     # rank 63 is group 0: it receives first
                for s in SENDERS:
                    for n in (BULK_N, 4097):
                        X.round([link(s, 63, mode, n, 20 if mode == NONBLOCKING else 5, **kw)],
                                ("descending", engine, kw, mode, s, n))
        counts = [X.c.link_counters(63, s) for s in SENDERS]
        assert all(a["rx_seq"] > b["rx_seq"] + 5000 and a["calls"] > b["calls"] + 50 for a, b in zip(counts, counts[1:]))
        if engine == "kernel":
            last = None
            for s in (37, 5, 21, 13):     # 37 then 5: equal modulo 32; 5 then 21: modulo 16; 21 then 13: modulo 8
                if last is not None:
                    X.advance(s, 63, seq_by=last - 1 - X.c.link_counters(63, s)["rx_seq"])
                out = X.round([link(s, 63, PINGPONG, 2045, 9, proto=PROTO_LL)], ("LL, equal tags", s))
                assert last is None or X.c.link_counters(63, s)["rx_seq"] == last + 8
                last = X.c.link_counters(63, s)["rx_seq"]
                assert out[63].recv_done == 9
    finally:
        X.close()


@pytest.mark.parametrize("case", ["credits", "unequal"])
def test_three_slot_rings_at_high_ranks_and_unequal_rings(case):
    """MPX_CHECK_RING_BYTES of two short slots, in a child (tests/ranks_worker.py)"""
    env = dict(os.environ, MPX_CHECK_RING_BYTES=str(CREDIT_RING))
    p = run_bounded([sys.executable, os.path.join(HERE, "ranks_worker.py"), case], env=env, timeout=100)
    assert p.returncode == 0 and p.stdout.split()[-1:] == ["ok"], (p.stdout[-400:], p.stderr[-2000:])


# ---- fan ----------------------------------------------------------------------
FAN_RANKS = [9, 63, 1, 40]                # rank 9 lists its peers in this order: 63, 1, 40
FAN_ALIASES = [9, 33, 1, 17]              # rank 9's peers are all 1 modulo 8 and 16, two of them modulo 32


@pytest.mark.parametrize("ranks", [FAN_RANKS, FAN_ALIASES], ids=["9-63-1-40", "9-33-1-17"])
@pytest.mark.parametrize("block_len,stride", [(2045, 2064), (BULK_N, BULK_N + 27)])
def test_fan_star_on_sparse_ranks(block_len, stride, ranks):
    """stride larger than block_len, block_len no multiple of 16; the whole
    of rx is compared, so the blocks of the 60 absent ranks and the gaps stay
    0xEE; every link reports the width mpx_fan_width gives a 64-rank context.
    The hub receives from all its peers inside one launch, its links at
    distinct counts."""
    hub, a, b, c = ranks
    fan = F.Fan(64, 64 * stride, ranks=ranks)
    try:
        fan.layout(block_len, stride)
        fan.advance([(hub, a)], seq_by=3000, calls_by=11)
        fan.advance([(hub, b)], seq_by=2000)
        fan.advance([(hub, c)], seq_by=1000, calls_by=2)
        w = mpx.fan_width(64, block_len)
        assert w == F.fan_width(64, block_len) and w >= 1
        star = {hub: [a, b, c], a: [hub], b: [hub], c: [hub]}
        fan.checked_call(star, 5, True, ("star checked", block_len), widths=w)
        fan.checked_call(star, 17, False, ("star unchecked", block_len), widths=w)
        ring = {hub: [c, a], a: [hub, b], b: [a, c], c: [b, hub]}
        fan.checked_call(ring, 3, True, ("ring", block_len), widths=w)
        fan.checked_call({a: [c], c: [a]}, 4, True, ("one link", block_len), widths=w)
    finally:
        fan.close()


def test_fan_length_checks_with_one_short_peer():
    """a fan call needs (highest rank + 1) * stride bytes attached on the
    caller and (caller + 1) * stride on every peer: rank 1 holds ten blocks"""
    block_len, stride = 2045, 2064
    fan = F.Fan(64, 64 * stride, ranks=FAN_RANKS, caps={1: 10 * stride})
    try:
        fan.layout(block_len, stride)
        fan.checked_call({9: [1], 1: [9]}, 5, True, "short peer, blocks 1 and 9")     # 10 * stride fits exactly
        fan.checked_call({9: [63, 40], 63: [9], 40: [9]}, 5, True, "the long ranks")
        rows = [(r, p) for r in FAN_RANKS for p in range(64) if p != r]
        before = {k: fan.counters(*k) for k in rows}
        refused = [({1: [40], 40: [1]}, "rank 1's own block 40 and rank 40's block for it lie past rank 1's ten blocks"),
                   ({63: [9, 1]}, "one short peer among long ones refuses the whole call"),
                   ({1: [9, 63]}, "one peer number too high for the caller's own length")]
        for peersets, what in refused:
            out, errs = fan.run(peersets, 5)
            assert not out and sorted(errs) == sorted(peersets), (what, out, errs)
            assert all(e.status == mpx.ERR_INVALID for e in errs.values()), (what, errs)
        # a stride 16 bytes longer: rank 1's length no longer holds block 9, for either side of the link
        fan.stride += 16
        try:
            out, errs = fan.run({9: [1], 1: [9]}, 5)
        finally:
            fan.stride -= 16
        assert not out and sorted(errs) == [1, 9], (out, errs)
        assert all(e.status == mpx.ERR_INVALID for e in errs.values()), errs
        fan.verify_bytes({}, "refused fan calls", moved=False)
        assert {k: fan.counters(*k) for k in rows} == before
        fan.checked_call({9: [1], 1: [9]}, 5, True, "the short link still works after the refusals")
    finally:
        fan.close()


# ---- two processes ---------------------------------------------------------------
def test_two_process_ipc_ranks_9_and_63(tmp_path):
    """ranks 9 (group 1) and 63 of a 64-rank context, one process each:
    RankDesc.rank, the peer's mailbox row 63 and this side's row 9 through IPC,
    pushed and pulled"""
    env = dict(os.environ, IPC_WORKER_RANKS="9,63", IPC_WORKER_NRANKS="64")
    worker = os.path.join(HERE, "ipc_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(tmp_path), str(i), "kernel-both"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for i in (0, 1)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=100)[0])
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate()[0])
    assert all(p.returncode == 0 for p in procs), outs
    for i, rank in enumerate((9, 63)):
        desc = (tmp_path / f"desc_{i}.bin").read_bytes()
        assert int.from_bytes(desc[12:16], "little", signed=True) == rank      # RankDesc: magic[8], abi, rank
        res = json.load(open(tmp_path / f"result_{i}.json"))
        assert len(res) == 2 * 3 * 8 and [x["pull"] for x in res] == [False] * 24 + [True] * 24
        pushes = 0
        for k, x in enumerate(res):
            pushes += x["iters"]
            assert x["final_rx_ok"], (rank, x)
            assert x["check_failures"] == 0 and x["check_iters"] == x["iters"], (rank, x)
            assert x["recv_done"] == (x["iters"] - x["iters"] // 256 if x["mode"] == 1 else x["iters"]), (rank, x)
            ll = x["mode"] != 1 and x["n"] <= 2048
            assert x["protocol"] == (0 if ll else 7 if x["pull"] else 1), (rank, x)
            assert x["counters"] == dict(tx_seq=pushes, rx_seq=pushes, calls=k + 1, token=k + 1), (rank, k, x)
            assert x["other_rows_zero"], (rank, k, x)


# ---- unequal ends of a link --------------------------------------------------------
SHORT = CREDIT_CAP      # 4097 + GUARD bytes


@pytest.mark.parametrize("engine", ["kernel", "sdma"])
def test_unequal_attached_lengths(engine):
    """rank 5 attached with 4097 + GUARD bytes, rank 63 with 1 MiB: calls up
    to the smaller length pass byte for byte in every mode and either group
    order (non-blocking check mode with the default rings here, with rings of
    different slot counts in tests/ranks_worker.py unequal); a longer
    buff_len is MPX_ERR_INVALID on both ranks and moves nothing"""
    X = Links(engine, [5, 63], 1 << 20, caps={5: SHORT})
    push, pull = (PROTO_BULK, PROTO_PULL) if engine == "kernel" else (PROTO_SDMA, PROTO_SDMA_PULL)
    try:
        X.advance(5, 63, seq_by=500, calls_by=4)
        digests = {}
        for a, b in ((5, 63), (63, 5)):
            for mode in (PINGPONG, UNIDIR, NONBLOCKING):
                iters = 300 if mode == NONBLOCKING else 9
                for n in (8, CREDIT_N, SHORT):
                    out = X.round([link(a, b, mode, n, iters)], ("unequal", engine, a, b, mode, n))
                    digests[(a, mode, n)] = {r: (out[r].recv_done, out[r].recv_digest) for r in (5, 63)}
                X.round([link(a, b, mode, SHORT, 9, proto=pull, pull=True)], ("unequal pulled", engine, a, b, mode))
                X.round([link(a, b, mode, SHORT, 9, check=False, proto=push)],
                        ("unequal unchecked", engine, a, b, mode))
                X.refused([link(a, b, mode, SHORT + 1, 9)], ("one byte past the short end", engine, a, b, mode))
                X.refused([link(a, b, mode, 1 << 20, 9, check=False, pull=True)],
                          ("the long length", engine, a, b, mode))
        # the symmetric loops give each rank the same receives whichever rank is group 1
        for mode in (PINGPONG, NONBLOCKING):
            for n in (8, CREDIT_N, SHORT):
                assert digests[(5, mode, n)] == digests[(63, mode, n)], (mode, n)
        X.round([link(5, 63, PINGPONG, SHORT, 9)], "the link still works after the refusals")
    finally:
        X.close()


@pytest.mark.parametrize("engine", ["kernel", "sdma"])
def test_group_order_inverted(engine):
    """the higher rank number as group 1, in ping-pong and unidir, checked:
    the same bytes, counts and digests per role as in the usual order"""
    n = 4097
    X = Links(engine, [5, 63], BULK_N + GUARD)
    try:
        for mode in (PINGPONG, UNIDIR):
            for size in (8, n, BULK_N):
                usual = X.round([link(5, 63, mode, size, 9)], ("usual order", engine, mode, size))
                inverted = X.round([link(63, 5, mode, size, 9)], ("inverted order", engine, mode, size))
                for g1, g0, out in ((5, 63, usual), (63, 5, inverted)):
                    assert out[g1].recv_done == out[g0].recv_done == 9
                    m = 1 if mode == UNIDIR else size       # what group 1 receives (mpi_perf.c:137,142)
                    assert out[g1].recv_digest == (9 * O.checksum(X.host[g0][:m])) & 0xFFFFFFFFFFFFFFFF
                    assert out[g0].recv_digest == (9 * O.checksum(X.host[g1][:size])) & 0xFFFFFFFFFFFFFFFF
                assert usual[5].protocol == usual[63].protocol == inverted[5].protocol == inverted[63].protocol
                assert usual[5].bytes == inverted[63].bytes and usual[5].nwg == inverted[63].nwg
    finally:
        X.close()
