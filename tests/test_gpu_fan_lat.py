"""The link recorder (mpx_fan_lat_*, k_xfer_fan_ll's traced form) on the GPU: loopback
ranks on GPU 0 (tests/fan_ll.py).

Lane 0 of every workgroup of a traced MPX_FAN_LL call — workgroup k IS link k —
reads the kernel's clock (10 ns ticks) once per iteration of its link's
lock-step loop and streams d = t[i+1] - t[i] into the block of that link's
PEER: min / max / sum / histogram, and the stamps into a raw trace.  With the
whole call inside the raw trace the streamed statistics must equal the same
statistics computed from the trace on the host — exactly, in integer ticks.
Every transfer goes through Fan.checked_call (host bytes, digests, link
counters from both sides): a traced call moves exactly what the untraced one
moves.  Every deadline is 5000 ms.
"""
import fnmatch
import glob
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import mpx
import oracle_py as O
import payload
from fan import full_mesh
from fan_ll import LLFan, mesh

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "fan_lat_worker.py")
TICK = 1e-8
MESH3 = full_mesh(3)
STAT_KEYS = ("count", "calls", "min_ticks", "max_ticks", "sum_ticks", "max_iter", "last_iters")
RESULT_FIELDS = ("recv_done", "recv_digest", "check_iters", "check_failures", "bytes", "protocol", "nwg", "launches")
LINK_FIELDS = ("peer", "nwg", "recv_done", "recv_digest", "check_failures")


def worker(args, mpx_test, timeout=60):
    p = subprocess.run([sys.executable, WORKER, *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, MPX_TEST=mpx_test))
    assert p.returncode == 0, (args, p.stdout[-600:], p.stderr[-1500:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def bucket_counts(d):
    return np.bincount([mpx.lat_bucket(int(x)) for x in d], minlength=mpx.LAT_BUCKETS).tolist()


def deltas(raw):
    return [b - a for a, b in zip(raw, raw[1:])]


def is_zero(lat):
    return all(lat[k] == 0 for k in STAT_KEYS) and not any(lat["hist"]) and lat["tick_s"] == TICK


def stats_equal_trace(lat, raw, iters, what, calls=1):
    """one traced call, whole inside the raw trace: the block's streamed
    statistics are the trace's own, in integer ticks"""
    assert len(raw) == iters + 1, (what, len(raw))
    d = deltas(raw)
    assert all(x >= 0 for x in d), (what, "stamps decrease")
    assert lat["count"] == iters and lat["calls"] == calls and lat["last_iters"] == iters, (what, lat)
    assert lat["tick_s"] == TICK
    assert (lat["min_ticks"], lat["max_ticks"], lat["sum_ticks"]) == (min(d), max(d), sum(d)), (what, lat, d)
    assert lat["sum_ticks"] == raw[-1] - raw[0], what                # the sum telescopes
    assert lat["hist"] == bucket_counts(d), what
    assert lat["max_iter"] == int(np.argmax(d)), (what, lat["max_iter"], d)   # the first maximum


def enable_all(F, ranks, raw_cap):
    for r in ranks:
        F.c.fan_lat_enable(r, raw_cap)


def check_every_link(F, sets, out, iters, what):
    for r, peers in sets.items():
        t, links = out[r]
        for k, p in enumerate(peers):
            lat, raw = F.c.fan_lat_get(r, p), F.c.fan_lat_raw(r, p)
            stats_equal_trace(lat, raw, iters, (what, r, p))
            # the link's iterations lie inside the call, by the host's clock
            assert lat["sum_ticks"] * TICK <= t.wall_s, (what, r, p, lat["sum_ticks"], t.wall_s)
            print(f"{what} link {r}-{p}: min {lat['min_ticks']} max {lat['max_ticks']} sum {lat['sum_ticks']} ticks, "
                  f"device_s - sum {links[k]['device_s'] - lat['sum_ticks'] * TICK:.3e} s")


def results(out, r):
    t, links = out[r]
    return {f: getattr(t, f) for f in RESULT_FIELDS}, [{f: l[f] for f in LINK_FIELDS} for l in links]


# ---- 1. streamed statistics equal the raw trace, per link ---------------------------
@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("n", [8, 4096])
def test_streamed_statistics_equal_the_raw_trace(n, check):
    F = mesh(3, n)
    try:
        for k, iters in enumerate((1, 2, 300)):
            if k:
                F.set_tx_seed(k)
            enable_all(F, MESH3, 512)                                # (resets)
            out = F.checked_call(MESH3, iters, check, ("trace", n, iters, check))
            check_every_link(F, MESH3, out, iters, f"B {n} iters {iters} check {check}")
    finally:
        F.close()


def test_push_count_odd_at_entry():
    """a 1-iteration call first: every link's push count is odd when the traced
    call starts, so its first push lands in the other half of the LL row"""
    F = mesh(3, 4096)
    try:
        F.checked_call(MESH3, 1, True, "first, untraced")
        assert all(F.counters(r, p)["tx_seq"] == 1 for r in MESH3 for p in MESH3[r])
        F.set_tx_seed(1)
        enable_all(F, MESH3, 512)
        out = F.checked_call(MESH3, 8, True, "odd at entry")
        check_every_link(F, MESH3, out, 8, "odd at entry")
    finally:
        F.close()


# ---- 2. raw cap ------------------------------------------------------------------------
def test_raw_trace_is_capped_and_the_statistics_are_not():
    F = mesh(3, 2049)
    try:
        enable_all(F, MESH3, 16)
        F.checked_call(MESH3, 40, True, "cap 16")
        for r, p in ((r, p) for r in MESH3 for p in MESH3[r]):
            raw, lat = F.c.fan_lat_raw(r, p), F.c.fan_lat_get(r, p)
            assert len(raw) == 17
            assert lat["count"] == 40 and sum(lat["hist"]) == 40 and lat["last_iters"] == 40
            part = bucket_counts(deltas(raw))
            assert all(a <= h for a, h in zip(part, lat["hist"]))
            assert F.c.fan_lat_raw(r, p, cap=5) == raw[:5]
        F.set_tx_seed(1)
        enable_all(F, MESH3, 0)
        F.checked_call(MESH3, 40, False, "cap 0")
        for r, p in ((r, p) for r in MESH3 for p in MESH3[r]):
            lat = F.c.fan_lat_get(r, p)
            assert F.c.fan_lat_raw(r, p) == []
            assert lat["count"] == 40 and sum(lat["hist"]) == 40 and lat["calls"] == 1
            assert 0 < lat["min_ticks"] <= lat["max_ticks"] <= lat["sum_ticks"]
    finally:
        F.close()


# ---- 3. accumulate, reset, disable ----------------------------------------------------
def test_accumulate_reset_disable():
    F = mesh(3, 8)
    links = [(r, p) for r in MESH3 for p in MESH3[r]]
    try:
        out = F.checked_call(MESH3, 50, True, "untraced")
        want = {r: results(out, r) for r in MESH3}
        enable_all(F, MESH3, 64)
        F.checked_call(MESH3, 50, True, "first")
        first = {l: F.c.fan_lat_get(*l) for l in links}
        F.checked_call(MESH3, 50, True, "second")
        for l in links:
            lat, raw = F.c.fan_lat_get(*l), F.c.fan_lat_raw(*l)
            assert lat["count"] == 100 and lat["calls"] == 2 and lat["last_iters"] == 50 and sum(lat["hist"]) == 100
            d = deltas(raw)                                          # the second call's
            assert len(raw) == 51
            assert lat["sum_ticks"] == first[l]["sum_ticks"] + sum(d)
            assert lat["min_ticks"] == min(first[l]["min_ticks"], min(d))
            assert lat["max_ticks"] == max(first[l]["max_ticks"], max(d))
            assert lat["hist"] == [a + b for a, b in zip(first[l]["hist"], bucket_counts(d))]
            assert lat["max_iter"] == (int(np.argmax(d)) if max(d) > first[l]["max_ticks"] else first[l]["max_iter"])
        for r in MESH3:
            F.c.fan_lat_reset(r)
            for p in MESH3[r]:                                       # every peer's block
                assert is_zero(F.c.fan_lat_get(r, p)) and F.c.fan_lat_raw(r, p) == []
        for r in MESH3:
            F.c.fan_lat_disable(r)
            for call in (lambda: F.c.fan_lat_get(r, MESH3[r][0]), lambda: F.c.fan_lat_raw(r, MESH3[r][0]),
                         lambda: F.c.fan_lat_reset(r)):
                with pytest.raises(mpx.MpxError) as e:
                    call()
                assert e.value.status == mpx.ERR_STATE
        out = F.checked_call(MESH3, 50, True, "after disable")
        assert {r: results(out, r) for r in MESH3} == want
    finally:
        F.close()


# ---- 4. keyed by peer, not by position ---------------------------------------------------
def test_blocks_are_keyed_by_peer_not_by_position():
    iters = 7
    F = mesh(4, 4095, 4096)                                         # rank 3: attached, never listed
    try:
        enable_all(F, range(4), 32)
        A = {0: [2, 1], 1: [0, 2], 2: [0, 1]}
        out = F.checked_call(A, iters, True, "A")
        for r, peers in A.items():
            for p in peers:
                stats_equal_trace(F.c.fan_lat_get(r, p), F.c.fan_lat_raw(r, p), iters, ("A", r, p))
        F.set_tx_seed(1)
        F.checked_call({0: [1], 1: [0]}, iters, True, "B")
        g01, g02, g12 = F.c.fan_lat_get(0, 1), F.c.fan_lat_get(0, 2), F.c.fan_lat_get(1, 2)
        assert g01["calls"] == 2 and g01["count"] == 2 * iters, g01
        assert g02["calls"] == 1 and g02["count"] == iters, g02
        assert g12["calls"] == 1 and g12["count"] == iters, g12
        assert F.c.fan_lat_get(1, 0)["calls"] == 2
        for r in range(3):
            assert is_zero(F.c.fan_lat_get(r, 3)) and F.c.fan_lat_raw(r, 3) == []
        for p in range(3):
            assert is_zero(F.c.fan_lat_get(3, p))
    finally:
        F.close()


# ---- 5. one end traced ------------------------------------------------------------------
def test_one_end_traced():
    F = mesh(3, 4096)
    try:
        F.c.fan_lat_enable(0, 64)
        out = F.checked_call(MESH3, 12, True, "rank 0 traced alone")
        for p in (1, 2):
            stats_equal_trace(F.c.fan_lat_get(0, p), F.c.fan_lat_raw(0, p), 12, ("one end", p))
        with pytest.raises(mpx.MpxError) as e:
            F.c.fan_lat_get(1, 0)
        assert e.value.status == mpx.ERR_STATE
    finally:
        F.close()


# ---- 6. a stall lands on its link and its iteration -----------------------------------------
def test_a_stall_lands_on_its_link_and_its_iteration():
    """MPX_TEST=lag_wg=1:0:20000 (a process of its own): rank 1's workgroup of
    link 0 (to rank 0) stalls 20 ms between its push and its wait of iteration
    10 of 20.  Rank 1's iteration 10 on that link takes the 20 ms.  Rank 1's
    push 10 left before the stall, so rank 0's iteration 10 is quick: it is
    push 11 that rank 0 waits 20 ms for.  The other four links run on
    workgroups of their own and see nothing of it."""
    res = worker(["lag"], "lag_wg=1:0:20000")
    assert res["ok"] and len(res["links"]) == 6, res
    for name, x in res["links"].items():
        lat = x["lat"]
        print(f"link {name}: max {lat['max_ticks']} ticks at iteration {lat['max_iter']}, "
              f"p50 {mpx.lat_quantile(lat, 0.5)}, deltas {deltas(x['raw'])}")
        stats_equal_trace(lat, x["raw"], 20, name)
    l10, l01 = res["links"]["1-0"]["lat"], res["links"]["0-1"]["lat"]
    assert l10["max_iter"] == 10
    assert l01["max_iter"] == 11
    for lat in (l10, l01):
        assert lat["max_ticks"] >= 2_000_000
        assert mpx.lat_quantile(lat, 0.5) < lat["max_ticks"]
    for r in ("0", "1"):
        assert res["wall_s"][r] >= 0.0196, res["wall_s"]
    for name, x in res["links"].items():
        if name not in ("1-0", "0-1"):
            assert x["lat"]["max_ticks"] < 1_000_000, (name, x["lat"]["max_ticks"])


# ---- 7. independence of the two recorders ------------------------------------------------------
def test_the_two_recorders_are_independent():
    from test_gpu_fan_ll import pair_call
    F = mesh(3, 8)
    links = [(r, p) for r in MESH3 for p in MESH3[r]]
    try:
        for r in MESH3:
            F.c.lat_enable(r, 16)
            F.c.fan_lat_enable(r, 16)
        F.checked_call(MESH3, 5, True, "LL fan, traced")
        snap = {l: (F.c.fan_lat_get(*l), F.c.fan_lat_raw(*l)) for l in links}
        assert all(s[0]["calls"] == 1 and s[0]["count"] == 5 for s in snap.values())
        # the LL fan call left the rank recorder alone
        for r in MESH3:
            lat = F.c.lat_get(r)
            assert lat["count"] == 0 and lat["calls"] == 0 and F.c.lat_raw(r) == []
        # a bulk fan call and a pair ping-pong leave every link block alone
        F.ll = False
        F.checked_call(MESH3, 5, True, "bulk fan")
        F.ll = True
        assert {l: (F.c.fan_lat_get(*l), F.c.fan_lat_raw(*l)) for l in links} == snap
        pair_call(F, mpx.MODE_PINGPONG, 8, 6, "pair ping-pong", 0)
        assert {l: (F.c.fan_lat_get(*l), F.c.fan_lat_raw(*l)) for l in links} == snap
        # and the pair call filled the rank recorder of its two ranks
        for r in (0, 1):
            lat = F.c.lat_get(r)
            assert lat["count"] == 6 and lat["calls"] == 1 and len(F.c.lat_raw(r)) == 7
        before = {r: F.c.lat_get(r) for r in MESH3}
        F.checked_call(MESH3, 4, True, "LL fan again")
        for r in MESH3:
            after = F.c.lat_get(r)
            assert (after["count"], after["calls"]) == (before[r]["count"], before[r]["calls"])
        assert all(F.c.fan_lat_get(*l)["calls"] == 2 for l in links)
    finally:
        F.close()


# ---- 8. status codes -----------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(mpx.MpxError) as e:
        call()
    return e.value.status


def test_other_engines_refuse_the_link_recorder():
    with mpx.Context(2, "sdma") as c:
        assert status_of(lambda: c.fan_lat_enable(0, 16)) == mpx.ERR_UNSUPPORTED


def test_invalid_arguments():
    F = LLFan(4, 4 * 16 + 4096, ranks=[0, 1, 2])                     # rank 3: not attached
    try:
        c = F.c
        for cap in (-1, mpx.FAN_LAT_RAW_MAX + 1):
            assert status_of(lambda: c.fan_lat_enable(0, cap)) == mpx.ERR_INVALID
        for call in (lambda: c.fan_lat_enable(3, 16), lambda: c.fan_lat_disable(3), lambda: c.fan_lat_reset(3),
                     lambda: c.fan_lat_get(3, 0), lambda: c.fan_lat_raw(3, 0),
                     lambda: c.fan_lat_enable(4, 16), lambda: c.fan_lat_enable(-1, 16)):
            assert status_of(call) == mpx.ERR_INVALID
        c.fan_lat_enable(0, 16)
        for peer in (0, 4, -1):
            assert status_of(lambda: c.fan_lat_get(0, peer)) == mpx.ERR_INVALID
            assert status_of(lambda: c.fan_lat_raw(0, peer)) == mpx.ERR_INVALID
        n = mpx.C.c_int(0)
        assert c.L.mpx_fan_lat_get(c.h, 0, 1, None) == mpx.ERR_INVALID
        assert c.L.mpx_fan_lat_raw(c.h, 0, 1, None, 4, mpx.C.byref(n)) == mpx.ERR_INVALID
        assert c.L.mpx_fan_lat_raw(c.h, 0, 1, None, 0, None) == mpx.ERR_INVALID
        assert is_zero(c.fan_lat_get(0, 3))                          # in range, never listed: zeros
    finally:
        F.close()


def test_armed_rank_refuses_all_five_and_the_armed_call_still_runs():
    F = mesh(3, 8)
    try:
        c = F.c
        c.fan_lat_enable(0, 16)
        iters = 4
        out, errs = {}, {}

        def args(r):
            h = F.host[1 - r]
            return ((mpx.MODE_PINGPONG, 1 if r == 0 else 0, r, 1 - r, iters, F.bufs[r][0], F.bufs[r][1], 8),
                    dict(check_payload=True, expect=O.checksum(h[:8]), expect_ack=O.checksum(h[:1]), timeout_ms=5000))

        a0, kw0 = args(0)
        c.arm(*a0, **kw0)
        try:
            for call in (lambda: c.fan_lat_enable(0, 16), lambda: c.fan_lat_disable(0), lambda: c.fan_lat_reset(0),
                         lambda: c.fan_lat_get(0, 1), lambda: c.fan_lat_raw(0, 1)):
                assert status_of(call) == mpx.ERR_STATE
        except BaseException:
            c.disarm(0)
            raise

        def side(r):
            a, kw = args(r)
            try:
                out[r] = c.xfer(*a, **kw)
            except mpx.MpxError as e:
                errs[r] = e

        th = [threading.Thread(target=side, args=(r,)) for r in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for r in (0, 1):
            assert out[r].check_failures == 0 and out[r].check_iters == iters and out[r].recv_done == iters
        assert c.phases(0)["armed"] == 1
        assert is_zero(c.fan_lat_get(0, 1))                          # a pair call: untouched
    finally:
        F.close()


def test_enabling_again_with_a_larger_cap_regrows():
    F = mesh(3, 4096)
    try:
        enable_all(F, MESH3, 4)
        F.checked_call(MESH3, 10, True, "cap 4")
        assert all(len(F.c.fan_lat_raw(r, p)) == 5 for r in MESH3 for p in MESH3[r])
        F.set_tx_seed(1)
        enable_all(F, MESH3, 2048)
        out = F.checked_call(MESH3, 600, True, "cap 2048")
        check_every_link(F, MESH3, out, 600, "regrown")
    finally:
        F.close()


def test_enabling_again_with_a_smaller_cap_keeps_the_blocks_apart():
    """cap 64, then cap 2: the allocation stays and the blocks' stride shrinks,
    for the host and the kernel alike — every link's block holds its own call.
    Three attached ranks in a context of four: rank 3 is never listed, so its
    block, the last at the new stride, reads zeros on every rank.  (A rank's OWN
    block has no reader: peer == rank is MPX_ERR_INVALID.)"""
    iters = 5
    F = LLFan(4, 4 * 16 + payload.GUARD, ranks=[0, 1, 2])
    F.layout(8, 16)
    try:
        enable_all(F, MESH3, 64)
        enable_all(F, MESH3, 2)
        F.checked_call(MESH3, iters, True, "cap 64, then 2")
        for r, p in ((r, p) for r in MESH3 for p in MESH3[r]):
            lat, raw = F.c.fan_lat_get(r, p), F.c.fan_lat_raw(r, p)
            assert len(raw) == 3 and raw[0] <= raw[1] <= raw[2], (r, p, raw)
            assert lat["count"] == iters and lat["calls"] == 1 and lat["last_iters"] == iters, (r, p, lat)
            assert sum(lat["hist"]) == iters and lat["sum_ticks"] >= raw[2] - raw[0], (r, p, lat)
        for r in MESH3:
            assert is_zero(F.c.fan_lat_get(r, 3)) and F.c.fan_lat_raw(r, 3) == []
            assert status_of(lambda: F.c.fan_lat_get(r, r)) == mpx.ERR_INVALID
    finally:
        F.close()


# ---- 9. iters = 0 ---------------------------------------------------------------------------------
def test_a_call_without_iterations():
    F = mesh(3, 4096)
    try:
        enable_all(F, MESH3, 16)
        F.checked_call(MESH3, 5, True, "five")
        before = {(r, p): F.c.fan_lat_get(r, p) for r in MESH3 for p in MESH3[r]}
        F.checked_call(MESH3, 0, True, "none")
        for (r, p), b in before.items():
            lat, raw = F.c.fan_lat_get(r, p), F.c.fan_lat_raw(r, p)
            assert lat["calls"] == b["calls"] + 1 == 2 and lat["last_iters"] == 0
            want = dict(b, calls=2, last_iters=0)
            assert lat == want, (r, p)
            assert len(raw) <= 1                                     # no stamp beyond t[0]
    finally:
        F.close()


# ---- 10. across a wrap ----------------------------------------------------------------------------
def test_across_the_push_counter_wrap():
    """every link 4 pushes short of 2^32, 9 traced and checked iterations (a
    process of its own: mpx_test_advance_link)"""
    res = worker(["wrap"], "")
    assert res["ok"] and len(res["links"]) == 6
    for name, x in res["links"].items():
        stats_equal_trace(x["lat"], x["raw"], 9, ("wrap", name))


# ---- 11. eight ranks x seven links ----------------------------------------------------------------
def test_eight_ranks_seven_links_each():
    sets = full_mesh(8)
    F = mesh(8, 8)
    try:
        enable_all(F, sets, 64)
        F.checked_call(sets, 33, True, "8 x 7")
        n = 0
        for r in sets:
            for p in sets[r]:
                lat = F.c.fan_lat_get(r, p)
                assert lat["count"] == 33
                stats_equal_trace(lat, F.c.fan_lat_raw(r, p), 33, ("8 x 7", r, p))
                n += 1
        assert n == 56
    finally:
        F.close()


# ---- 12. mpx_perf -m 2 -P ---------------------------------------------------------------------------
LAT_HEADER = ("Timestamp,JobId,Rank,PeerRank,Mode,BufferSize,NumOfBuffers,RunId,Count,MinUs,P50Us,P90Us,P99Us,P999Us,"
              "MaxUs,MeanUs,MaxIter")


def test_mpx_perf_writes_one_line_per_link(tmp_path):
    from test_gpu_host import run
    args = ["-w", "3", "-m", "2", "-c", "2", "-r", "3", "-i", "5", "-b", "2049", "-f", "@G1", "-n", "1", "-p", "1", "-l", "@LOGS"]
    (tmp_path / "plain").mkdir()
    (tmp_path / "lat").mkdir()
    p0, recs0, side0 = run(tmp_path / "plain", args, names="vm,runsc,runsc", gpus="0,0,0")
    assert p0.returncode == 0, p0.stderr[-800:]
    assert not glob.glob(str(tmp_path / "plain" / "logs" / "lat-*"))
    p, recs, side = run(tmp_path / "lat", args + ["-P", "64"], names="vm,runsc,runsc", gpus="0,0,0")
    assert p.returncode == 0, p.stderr[-800:]
    # the records and the gpu-*.csv lines have the shape they have without -P
    assert len(recs) == len(recs0) == 3 * 2 and len(side) == len(side0) == 2 * 6

    def shape(rs, keep):
        return sorted(tuple(f[i] for i in keep) for f in rs)
    assert shape(recs, (2, 3, 4, 5, 6, 7, 8, 10)) == shape(recs0, (2, 3, 4, 5, 6, 7, 8, 10))
    keep = (2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18, 19, 20)
    assert shape(side, keep) == shape(side0, keep)
    files = sorted(glob.glob(str(tmp_path / "lat" / "logs" / "lat-*.csv")))
    assert len(files) == 3
    for r, f in enumerate(files):
        name = os.path.basename(f)
        m = re.fullmatch(r"lat-([0-9a-f-]{36})-(\d)-\d{4}-\d\d-\d\d-\d\d-\d\d-\d\d\.csv", name)
        assert m and int(m.group(2)) == r, name
        assert not fnmatch.fnmatch(name, "tcp*") and not fnmatch.fnmatch(name, "gpu-*.csv")   # kusto_ingest.py skips it
        lines = open(f).read().splitlines()
        assert lines[0] == LAT_HEADER
        rows = [dict(zip(LAT_HEADER.split(","), x.split(","))) for x in lines[1:]]
        assert len(rows) == 2 * 2
        for run_id in (1, 2):
            mine = [x for x in rows if int(x["RunId"]) == run_id]
            assert sorted(int(x["PeerRank"]) for x in mine) == [q for q in range(3) if q != r]
        for x in rows:
            assert x["JobId"] == m.group(1) and int(x["Rank"]) == r and int(x["Mode"]) == 10
            assert (int(x["BufferSize"]), int(x["NumOfBuffers"]), int(x["Count"])) == (2049, 5, 5)
            mn, p50, p90, p99, p999, mx = (float(x[k]) for k in ("MinUs", "P50Us", "P90Us", "P99Us", "P999Us", "MaxUs"))
            assert 0 < mn <= p50 <= p90 <= p99 <= p999 <= mx
            assert mn <= float(x["MeanUs"]) <= mx and 0 <= int(x["MaxIter"]) < 5
