"""Sequenced fan payloads (mpx_xfer_fan_seq, include/mpx_fan_seq.h) on the GPU:
loopback ranks on GPU 0, a thread per rank (tests/fan_seq.py, tests/fan.py).

Every expectation is host bytes: the block rank s pushes to rank d in
iteration i is oracle_py.fill(n, FILL_SPLITMIX, mpx.pattern_key(seed, s, d,
i)).  rx is 0xEE before every call, guards and gaps included (the stride is
larger than the block), and the whole of rx and tx is read back after it.
Every call has a deadline of at most 5000 ms, which none is expected to use.
"""
import json
import os
import subprocess
import sys

import pytest

import fan_seq as S
import mpx
import oracle_py as O
import payload
from fan import M64, fan_width, full_mesh, round16
from payload import chunk_shape

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PINGPONG, NONBLOCKING = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING
BIG = (256 << 10) + 21
P31, P32 = 1 << 31, 1 << 32


# ---- 1. bulk: sizes, iteration counts, widths ---------------------------------------
@pytest.mark.parametrize("check", [True, False], ids=["check", "plain"])
@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 2045, 4161, BIG])
def test_bulk_sizes_and_iteration_counts(n, nranks, check):
    """a full mesh: the 16-byte unit and its tail, more than one chunk (4161:
    5 workgroups per link), and 33 iterations: the 16-push publish schedule
    with a mid-loop flag either side"""
    sets = full_mesh(nranks)
    F = S.mesh(nranks, n)
    try:
        for iters in (1, 3, 33):
            S.verified(F, sets, iters, ("bulk", n, nranks, check, iters), check=check, widths=fan_width(nranks, n))
    finally:
        F.close()


@pytest.mark.parametrize("check", [True, False], ids=["check", "plain"])
def test_bulk_stream(check):
    F = S.mesh(4, 4161)
    try:
        S.verified(F, full_mesh(4), 3, ("stream", check), check=check, stream=True)
    finally:
        F.close()


@pytest.mark.parametrize("check", [True, False], ids=["check", "plain"])
@pytest.mark.parametrize("nwg,n,nranks", [(7, 4161, 2), (7, 6421, 2), (70, 71681, 4), (1, BIG, 2)])
def test_bulk_explicit_widths(nwg, n, nranks, check):
    """7 at 4161 B is narrowed to 5 (at least 1 KiB per workgroup); 7 at 6421 B
    runs 7 wide: chunks of 928 B, the last 853 B with a 5-byte tail.  70 at 71681 B: chunks of 1040 B, workgroup 69 empty (it generates
    nothing and still publishes, credits and counts), workgroup 68 short; three
    links make a grid of 210.  1 at 256 KiB + 21: one workgroup walks the whole
    block, 4-deep batches and the tail"""
    if nwg == 70:
        assert chunk_shape(nwg, n) == (70, 1040, 1, 68, 961)
    if n == 6421:
        assert chunk_shape(nwg, n) == (7, 928, 0, 6, 853)
    width = fan_width(nranks, n, nwg=nwg)
    assert width == min(nwg, -(-n // 1024))
    F = S.mesh(nranks, n)
    try:
        for iters in (1, 3):
            S.verified(F, full_mesh(nranks), iters, ("widths", nwg, n, check, iters), check=check, widths=width, nwg=nwg)
    finally:
        F.close()


# ---- 2. peer sets ---------------------------------------------------------------------
@pytest.mark.parametrize("check", [True, False], ids=["check", "plain"])
def test_three_of_four_ranks(check):
    """the outsider's block and the rank's own block stay 0xEE, and rank 3's rx whole"""
    sets = {r: [p for p in range(3) if p != r] for r in range(3)}
    F = S.mesh(4, 2045)
    try:
        S.verified(F, sets, 3, ("3 of 4", check), check=check)
    finally:
        F.close()


@pytest.mark.parametrize("check", [True, False], ids=["check", "plain"])
def test_star(check):
    """a hub with three leaves: a leaf has one link, and every link a key of its own"""
    sets = {0: [3, 1, 2], 1: [0], 2: [0], 3: [0]}
    F = S.mesh(4, 4161)
    try:
        S.verified(F, sets, 3, ("star", check), check=check)
        assert len({S.sent(S.SEED, s, d, 2, 4161) for s in sets for d in sets[s]}) == 6
    finally:
        F.close()


@pytest.mark.parametrize("ll", [False, True], ids=["bulk", "ll"])
def test_high_rank_slots(ll):
    """ranks 9, 40 and 63 of a 64-rank context: src << 56 and dst << 48 of the key"""
    ranks = [9, 40, 63]
    sets = {r: [p for p in ranks if p != r] for r in ranks}
    F = S.mesh(64, 2045, ranks=ranks)
    try:
        S.verified(F, sets, 3, ("slots", ll), check=True, ll=ll)
    finally:
        F.close()


def test_eight_ranks_seven_links():
    F = S.mesh(8, 2045)
    try:
        S.verified(F, full_mesh(8), 3, "8 x 7", check=True)
    finally:
        F.close()


@pytest.mark.parametrize("ll", [False, True], ids=["bulk", "ll"])
def test_every_rank_lists_its_peers_in_another_order(ll):
    """expect[] and links[] follow the caller's order (S.verify holds both to it)"""
    sets = {0: [3, 1, 2], 1: [2, 0, 3], 2: [0, 3, 1], 3: [1, 2, 0]}
    F = S.mesh(4, 2045)
    try:
        S.verified(F, sets, 3, ("orders", ll), check=True, ll=ll)
    finally:
        F.close()


# ---- 3. the lock-step LL fan ----------------------------------------------------------
@pytest.mark.parametrize("check", [True, False], ids=["check", "plain"])
@pytest.mark.parametrize("nranks", [2, 4, 8], ids=["1link", "3links", "7links"])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 2045, 4095, 4096])
def test_ll_sizes_iteration_counts_and_halves(n, nranks, check):
    """every shape twice: with the link's first push in one half of the LL row
    and in the other (after an even count, a 1-iteration call in between)"""
    sets = full_mesh(nranks)
    F = S.mesh(nranks, n, stride=max(16, round16(n)) + 16)
    try:
        for iters in (1, 2, 3, 33):
            first = F.counters(0, 1)["tx_seq"] + 1
            S.verified(F, sets, iters, ("ll", n, nranks, check, iters, "a"), check=check, ll=True)
            if iters % 2 == 0:
                S.verified(F, sets, 1, ("ll", n, nranks, check, iters, "between"), check=check, ll=True)
            second = F.counters(0, 1)["tx_seq"] + 1
            assert (first ^ second) & 1      # the other half
            S.verified(F, sets, iters, ("ll", n, nranks, check, iters, "b"), check=check, ll=True)
    finally:
        F.close()


# ---- 4. check-mode bookkeeping ----------------------------------------------------------
@pytest.mark.parametrize("ll", [False, True], ids=["bulk", "ll"])
def test_expectations_are_per_link_and_iteration(ll):
    n, iters = 2045, 5
    sets = full_mesh(3)
    F = S.mesh(3, n)
    try:
        good = {r: S.expectations(r, sets[r], n, iters) for r in sets}
        # two entries of link 1 swapped (iterations 1 and 3): exactly those two fail, on that link alone
        bad = {r: list(good[r]) for r in sets}
        for r in sets:
            a, b = 1 * iters + 1, 1 * iters + 3
            bad[r][a], bad[r][b] = bad[r][b], bad[r][a]
        out, errs = S.run(F, sets, iters, expect=bad, ll=ll)
        assert not out and sorted(errs) == [0, 1, 2], (out, errs)
        for r, e in errs.items():
            assert e.status == mpx.ERR_CHECK and e.timing.check_failures == 2 and e.timing.check_iters == 2 * iters, (r, str(e))
            assert [l["check_failures"] for l in e.links] == [0, 2], (r, e.links)
            assert [l["recv_digest"] for l in e.links] == [sum(good[r][k * iters:(k + 1) * iters]) & M64 for k in (0, 1)], r
        S.verify_bytes(F, sets, iters - 1, "swapped")       # the transfer itself was whole
        # every entry iteration 0's checksum: every later iteration fails
        zero = {r: [good[r][k * iters] for k in range(2) for _ in range(iters)] for r in sets}
        out, errs = S.run(F, sets, iters, expect=zero, ll=ll)
        for r, e in errs.items():
            assert e.status == mpx.ERR_CHECK and [l["check_failures"] for l in e.links] == [iters - 1] * 2, (r, e.links)
            assert e.timing.check_failures == 2 * (iters - 1), r
        assert sorted(errs) == [0, 1, 2]
        # expect = None: the library computes them, and agrees with the host's
        out = S.verified(F, sets, iters, ("library's expectations", ll), expect=None, ll=ll)
        assert all(out[r][0].check_iters == 2 * iters for r in sets)
    finally:
        F.close()


def test_auto_max_refusal_moves_nothing():
    n = 4161
    iters = (mpx.SEQ_AUTO_MAX // n) + 1
    F = S.mesh(2, n)
    try:
        F.prefill()
        before = {(r, 1 - r): F.counters(r, 1 - r) for r in (0, 1)}
        with pytest.raises(mpx.MpxError) as ei:
            F.c.xfer_fan_seq(0, [1], iters, *F.bufs[0], n, F.stride, S.SEED, check_payload=True, expect=None, timeout_ms=2000)
        assert ei.value.status == mpx.ERR_INVALID and "MPX_SEQ_AUTO_MAX" in str(ei.value), str(ei.value)
        assert before == {k: F.counters(*k) for k in before}
        S.verify_bytes(F, {}, -1, "refused")
        # one iteration fewer is within the limit, and the caller's own array has none
        assert (iters - 1) * n <= mpx.SEQ_AUTO_MAX
        S.verified(F, full_mesh(2), 3, "after the refusal")
    finally:
        F.close()


# ---- 5. lost payloads (MPX_TEST in a process of its own) --------------------------------
@pytest.mark.parametrize("kind,k", [("bulk", 3), ("bulk", 2), ("ll", 2)])
def test_a_lost_payload_shows(kind, k):
    """skip_push=3, unchecked: iteration 1's payload is in every rx block —
    constant payloads cannot show this loss.  skip_push=2, checked: exactly
    one failure per link"""
    env = dict(os.environ, MPX_TEST=f"skip_push={k}")
    p = subprocess.run([sys.executable, os.path.join(HERE, "fan_seq_worker.py"), "lost", kind], capture_output=True,
                       text=True, env=env, timeout=120)
    assert p.returncode == 0 and json.loads(p.stdout.strip().splitlines()[-1])["ok"], (p.stdout[-400:], p.stderr[-1500:])


# ---- 6. mixing ----------------------------------------------------------------------------
def _counters(F):
    return {(r, p): F.counters(r, p) for r in F.ranks for p in F.ranks if p != r}


def test_alternating_with_ordinary_fan_and_pair_calls():
    """sequenced fan, ordinary fan, sequenced pair and ordinary pair calls on
    the links of one context, bulk and LL; the link counters after each"""
    n, iters = 2045, 3
    sets = full_mesh(3)
    F = S.mesh(3, n)
    tx = {r: F.bufs[r][0] for r in F.ranks}
    rx = {r: F.bufs[r][1] for r in F.ranks}
    try:
        import threading

        def pair(seq):
            """ranks 0 and 1, ping-pong, unchecked: rx[0 : n) gets the peer's message"""
            F.prefill()
            errs = []

            def side(r):
                try:
                    if seq:
                        F.c.xfer_seq(PINGPONG, 1 - r, r, 1 - r, iters, tx[r], rx[r], n, S.SEED + 1, timeout_ms=5000)
                    else:
                        F.c.xfer(PINGPONG, 1 - r, r, 1 - r, iters, tx[r], rx[r], n, timeout_ms=5000)
                except mpx.MpxError as e:
                    errs.append((r, str(e)))
            th = [threading.Thread(target=side, args=(r,)) for r in (0, 1)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not errs, errs
            for r in (0, 1):
                want = S.sent(S.SEED + 1, 1 - r, r, iters - 1, n) if seq else F.host[1 - r][:n]
                payload.assert_region(F.c, rx[r], 0, want, what=f"pair call, seq={seq}, rank {r}")

        for step, ll in enumerate([False, True, False, True]):
            S.verified(F, sets, iters, ("mixed, sequenced", step), check=step % 2 == 0, ll=ll)
            out, errs = F.run(sets, iters, check=True, ll=ll)
            assert not errs, errs
            F.verify_bytes(sets, ("mixed, ordinary", step))
            before = _counters(F)
            assert before[(0, 2)]["tx_seq"] == before[(0, 2)]["rx_seq"] == 2 * (step + 1) * iters, before[(0, 2)]
            pair(seq=True)
            pair(seq=False)
            after = _counters(F)
            for (r, p), b in before.items():
                on = {r, p} == {0, 1}
                assert after[(r, p)]["tx_seq"] == b["tx_seq"] + (2 * iters if on else 0), (r, p)
                assert after[(r, p)]["calls"] == b["calls"] + (2 if on else 0), (r, p)
        c01, c02 = F.counters(0, 1), F.counters(0, 2)
        assert c01["tx_seq"] == c01["rx_seq"] == 16 * iters and c01["calls"] == 16, c01
        assert c02["tx_seq"] == c02["rx_seq"] == 8 * iters and c02["calls"] == 8, c02
    finally:
        F.close()


@pytest.mark.parametrize("ll", [False, True], ids=["bulk", "ll"])
def test_only_one_rank_sequenced(ll):
    """unchecked, rank 0 alone calls mpx_xfer_fan_seq: both kinds of call
    complete; rank 0 receives its peers' tx blocks, they its payloads"""
    n, iters = 2045, 3
    sets = full_mesh(3)
    F = S.mesh(3, n)
    try:
        out, errs = S.run(F, sets, iters, check=False, seq_ranks=[0], ll=ll)
        assert not errs and all(out[r][0].recv_done == 2 * iters for r in sets), (out, errs)
        for r in sets:
            want = bytearray([payload.GUARD_BYTE]) * F.cap
            for p in sets[r]:
                want[p * F.stride:p * F.stride + n] = S.sent(S.SEED, 0, r, iters - 1, n) if p == 0 else F.block(p, r)
            payload.compare(F.c.read(F.bufs[r][1], F.cap), bytes(want), 0, f"one end sequenced: rx of rank {r}")
            payload.compare(F.c.read(F.bufs[r][0], F.cap), F.host[r], 0, f"one end sequenced: tx of rank {r}")
    finally:
        F.close()


# ---- 7. the link recorder -----------------------------------------------------------------
def test_sequenced_ll_calls_are_untraced_and_leave_the_recorder():
    n, iters = 2045, 5
    sets = full_mesh(3)
    F = S.mesh(3, n)
    try:
        for r in sets:
            F.c.fan_lat_enable(r, 64)
        out, errs = F.run(sets, iters, check=True, ll=True)      # traced, ordinary
        assert not errs, errs
        rec = {(r, p): F.c.fan_lat_get(r, p) for r in sets for p in sets[r]}
        raw = {(r, p): F.c.fan_lat_raw(r, p) for r in sets for p in sets[r]}
        assert all(v["count"] == iters and v["calls"] == 1 for v in rec.values()), rec
        S.verified(F, sets, iters, "sequenced under the recorder", ll=True)
        S.verified(F, sets, 2, "sequenced under the recorder, unchecked", check=False, ll=True)
        assert rec == {k: F.c.fan_lat_get(*k) for k in rec}
        assert raw == {k: F.c.fan_lat_raw(*k) for k in raw}
        out, errs = F.run(sets, iters, check=True, ll=True)      # and tracing goes on
        assert not errs and all(F.c.fan_lat_get(*k)["calls"] == 2 for k in rec), errs
    finally:
        F.close()


# ---- 8. counter wraps ---------------------------------------------------------------------
LINKS3 = [(0, 1), (0, 2), (1, 2)]


def test_ll_across_push_2pow31():
    """links 4 pushes short of 2^31, where the LL tag restarts"""
    F = S.mesh(3, 2045)
    try:
        for l in LINKS3:
            F.jump(l, P31 - 4)
        S.verified(F, full_mesh(3), 9, "LL across 2^31", check=True, ll=True)
        assert all(F.counters(*l)["tx_seq"] == P31 + 4 for l in LINKS3)
    finally:
        F.close()


def test_bulk_across_push_2pow32():
    F = S.mesh(3, 65555)
    try:
        for l in LINKS3:
            F.jump(l, P32 - 4)
        S.verified(F, full_mesh(3), 9, "bulk across 2^32", check=True, widths=5)
        assert all(F.counters(*l)["tx_seq"] == P32 + 4 for l in LINKS3)
    finally:
        F.close()


# ---- 9. two processes over IPC ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bulk", "ll"])
def test_two_processes(tmp_path, kind):
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fan_seq_worker.py"), "ipc", kind, str(tmp_path), str(p)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for p in (0, 1)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=100))
        except subprocess.TimeoutExpired:
            p.kill()
            outs.append(p.communicate())
    assert all(p.returncode == 0 for p in procs), outs
    iters = 5 if kind == "ll" else 3
    for p in (0, 1):
        x = json.loads(outs[p][0].strip().splitlines()[-1])
        assert x["rank"] == p and x["tx_ok"] and x["digest_ok"], x
        assert x["protocol"] == S.PROTO[kind == "ll"] and x["launches"] == 1, x
        assert x["check_failures"] == 0 and x["check_iters"] == iters == x["recv_done"], x
        assert x["after"]["tx_seq"] == x["before"]["tx_seq"] + iters and x["after"]["calls"] == x["before"]["calls"] + 1, x


# ---- 10. mpx_perf -Q 1 --------------------------------------------------------------------
BASE = ["-w", "3", "-f", "@G1", "-n", "1", "-p", "1", "-l", "@LOGS"]


@pytest.mark.parametrize("args,B,iters,proto", [(["-m", "1", "-i", "5", "-b", "65555", "-r", "3"], 65555, 5, "fan"),
                                                (["-m", "2", "-i", "5", "-b", "2045", "-r", "3"], 2045, 5, "fan_ll")],
                         ids=["m1", "m2"])
def test_mpx_perf_Q1(tmp_path, args, B, iters, proto):
    """every run one sequenced fan call; -c 1: every payload checked, and each
    link line's digest is that of the payloads the run's seed gives, from host
    bytes.  -c 0: the run completes"""
    from test_gpu_host import run
    d1, d0 = tmp_path / "c1", tmp_path / "c0"
    d1.mkdir()
    d0.mkdir()
    p, recs, side = run(d1, BASE + args + ["-Q", "1", "-c", "1"], names="vm,runsc,runsc", gpus="0,0,0")
    assert p.returncode == 0, p.stderr[-800:]
    assert len(recs) == 3 * 2 and len(side) == 2 * 6, (recs, side)
    for f in side:
        r, peer, run_idx = int(f[2]), int(f[6]), int(f[17])
        assert f[3] == "kernel" and f[13] == proto and int(f[8]) == B and int(f[9]) == iters, f
        assert int(f[15]) == iters and int(f[16]) == 0 and int(f[18]) == iters, f
        seed = (mpx.PATTERN_SEED + run_idx * 0x9E3779B97F4A7C15) & M64
        assert int(f[19]) == sum(S.csum(seed, peer, r, i, B) for i in range(iters)) & M64, f
    p, recs, side = run(d0, BASE + args + ["-Q", "1", "-c", "0"], names="vm,runsc,runsc", gpus="0,0,0")
    assert p.returncode == 0, p.stderr[-800:]
    assert len(recs) == 3 * 2 and all(int(f[15]) == 0 and int(f[18]) == iters for f in side), side


# ---- 11. refusals -------------------------------------------------------------------------
def _status(F, r, peers, iters=3, block_len=None, stride=None, seed=S.SEED, **kw):
    try:
        F.c.xfer_fan_seq(r, peers, iters, F.bufs[r][0], F.bufs[r][1], F.block_len if block_len is None else block_len,
                         F.stride if stride is None else stride, seed, timeout_ms=2000, **kw)
    except mpx.MpxError as e:
        return e.status
    return mpx.OK


def test_refusals_leave_the_rank_usable():
    """every refusal of the header's comment: its status, before any GPU work
    (the peers do not call), no number taken from a link, rx untouched, and a
    valid call follows"""
    import ctypes as C
    n = 4161
    sets = full_mesh(3)
    big = 262144
    F = S.Fan(3, 3 * big + payload.GUARD)
    try:
        F.layout(n, round16(n) + 16)
        F.prefill()
        before = _counters(F)
        L, h = F.c.L, F.c.h
        t, o = mpx.Timing(), mpx.FanSeqOpts(seed=1, timeout_ms=2000)
        arr = (C.c_int * 2)(1, 2)
        a = (0, 2, arr, 3, C.c_void_p(F.bufs[0][0].ptr), C.c_void_p(F.bufs[0][1].ptr), n, F.stride)
        assert L.mpx_xfer_fan_seq(None, *a, C.byref(o), C.byref(t), None) == mpx.ERR_INVALID
        assert L.mpx_xfer_fan_seq(h, 0, 2, None, *a[3:], C.byref(o), C.byref(t), None) == mpx.ERR_INVALID
        assert L.mpx_xfer_fan_seq(h, *a, None, C.byref(t), None) == mpx.ERR_INVALID
        assert L.mpx_xfer_fan_seq(h, *a, C.byref(o), None, None) == mpx.ERR_INVALID
        assert (mpx.XFER_STREAM, mpx.XFER_FAN_LL) == (1, 8)
        for flags in (2, 4, 16, mpx.XFER_FAN_LL | 4, mpx.XFER_STREAM | 2, 1 << 30):   # any other bit
            assert flags & ~(mpx.XFER_STREAM | mpx.XFER_FAN_LL)
            o2 = mpx.FanSeqOpts(seed=1, flags=flags, timeout_ms=2000)
            assert L.mpx_xfer_fan_seq(h, *a, C.byref(o2), C.byref(t), None) == mpx.ERR_INVALID, flags
        # whatever mpx_xfer_fan refuses, with its status
        assert _status(F, 0, [1, 1]) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 0]) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 3]) == mpx.ERR_INVALID
        assert _status(F, 0, []) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], iters=-1) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], stride=F.stride + 8) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], stride=round16(n) - 16) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], block_len=big, stride=big + 4096) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], block_len=big, stride=big, nwg=200) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], nwg=257) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], block_len=4112, stride=4112, ll=True) == mpx.ERR_INVALID      # above MPX_FAN_LL_MAX
        assert _status(F, 0, [1, 2], ll=True, stream=True) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], ll=True, nwg=2) == mpx.ERR_INVALID
        assert before == _counters(F)
        S.verify_bytes(F, {}, -1, "after the refusals")
        F.c.arm(PINGPONG, 1, 0, 1, 2, F.bufs[0][0], F.bufs[0][1], 4097, timeout_ms=2000)
        armed = F.counters(0, 1)
        assert _status(F, 0, [1, 2]) == mpx.ERR_STATE
        assert F.counters(0, 1) == armed
        F.c.disarm(0)
        S.verified(F, sets, 3, "a valid call after the refusals")
    finally:
        F.close()
    X = S.Fan(2, 2 * (round16(n) + 16) + payload.GUARD, engine="sdma")
    try:
        X.block_len, X.stride = n, round16(n) + 16
        assert _status(X, 0, [1]) == mpx.ERR_UNSUPPORTED
    finally:
        X.close()
