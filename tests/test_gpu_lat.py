"""The per-iteration latency recorder (mpx_lat_*, k_xfer_lat / k_xfer_pull_lat)
on the GPU: loopback pairs on GPU 0 (tests/pairs.py).

Workgroup 0 of a traced call reads the kernel's clock (10 ns ticks) once per
iteration and streams d = t[i+1] - t[i] into min / max / sum / histogram, and
the stamps themselves into a raw trace.  With the whole call inside the raw
trace, the streamed statistics must equal the same statistics computed from
the trace on the host — exactly, in integer ticks — and the stamps must sit
where mpx_phases says the first iteration and the loop end.  A traced call
must move, count and digest what the untraced call does.
"""
import fnmatch
import glob
import os
import re

import numpy as np
import pytest

import mpx
from pairs import Pairs
from proc import run_bounded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERF = os.path.join(ROOT, "mpi-perf_amd", "bin", "mpx_perf")

B_LL, B_BULK = 8, 65536 + 13
TICK = 1e-8
RESULT_FIELDS = ("recv_done", "recv_digest", "check_iters", "check_failures", "bytes", "protocol", "nwg")


@pytest.fixture(scope="module")
def pair():
    P = Pairs("kernel", 1, B_BULK)
    yield P
    P.close()


_untraced = {}


def untraced(P, mode, n, iters, pull):
    """the same call with no recorder: computed once per shape"""
    key = (mode, n, iters, pull)
    if key not in _untraced:
        for r in (0, 1):
            P.c.lat_disable(r)
        out, errs = P.run(mode, n, iters, pull=pull)
        assert not errs, errs
        _untraced[key] = {r: {f: getattr(out[r], f) for f in RESULT_FIELDS} for r in (0, 1)}
    return _untraced[key]


def traced(P, mode, n, iters, pull, raw_cap, **kw):
    for r in (0, 1):
        P.c.lat_enable(r, raw_cap)
    out, errs = P.run(mode, n, iters, pull=pull, **kw)
    assert not errs, errs
    return out


def bucket_counts(d):
    return np.bincount([mpx.lat_bucket(int(x)) for x in d], minlength=mpx.LAT_BUCKETS).tolist()


@pytest.mark.parametrize("iters", [1, 2, 300])
@pytest.mark.parametrize("n", [B_LL, B_BULK])
@pytest.mark.parametrize("pull", [False, True])
@pytest.mark.parametrize("mode", [mpx.MODE_PINGPONG, mpx.MODE_UNIDIR])
def test_streamed_statistics_equal_the_raw_trace(pair, mode, pull, n, iters):
    P = pair
    want = untraced(P, mode, n, iters, pull)
    out = traced(P, mode, n, iters, pull, 512)
    for r in (0, 1):
        raw = P.c.lat_raw(r)
        lat = P.c.lat_get(r)
        ph = P.c.phases(r)
        assert len(raw) == iters + 1
        d = [b - a for a, b in zip(raw, raw[1:])]
        print(f"mode {mode} pull {pull} B {n} iters {iters} rank {r}: min {min(d)} max {max(d)} sum {sum(d)} ticks, "
              f"first_iter_s {ph['first_iter_s']:.3e} kernel_s {ph['kernel_s']:.3e} tail_s {ph['tail_s']:.3e}")
        assert all(x >= 0 for x in d), "stamps decrease"
        assert lat["count"] == iters and lat["calls"] == 1 and lat["last_iters"] == iters
        assert lat["tick_s"] == TICK
        assert (lat["min_ticks"], lat["max_ticks"], lat["sum_ticks"]) == (min(d), max(d), sum(d))
        assert lat["hist"] == bucket_counts(d)
        assert lat["max_iter"] == int(np.argmax(d))            # the first maximum
        # where the stamps stand: t[0] is the instant first_iter_s counts from and
        # t[1] the kTsFirst stamp itself; t[iters] is taken inside the loop, which
        # workgroup 0 leaves (kTsLoop, where tail_s starts) no earlier
        assert abs(d[0] * TICK - ph["first_iter_s"]) < 0.5e-8
        assert lat["sum_ticks"] * TICK <= ph["kernel_s"] - ph["tail_s"] + 0.5e-8
        # the transfer itself: what the untraced call moved, counted and digested
        got = {f: getattr(out[r], f) for f in RESULT_FIELDS}
        assert got == want[r] and got["check_failures"] == 0 and got["check_iters"] == iters, (r, got, want[r])


@pytest.mark.parametrize("mode", [mpx.MODE_PINGPONG, mpx.MODE_UNIDIR])
def test_raw_trace_is_capped_and_the_statistics_are_not(pair, mode):
    P = pair
    traced(P, mode, B_BULK, 40, False, 16)
    for r in (0, 1):
        raw, lat = P.c.lat_raw(r), P.c.lat_get(r)
        assert len(raw) == 17
        assert lat["count"] == 40 and sum(lat["hist"]) == 40 and lat["last_iters"] == 40
        part = bucket_counts([b - a for a, b in zip(raw, raw[1:])])
        assert all(p <= h for p, h in zip(part, lat["hist"]))
        assert P.c.lat_raw(r, cap=5) == raw[:5]
    traced(P, mode, B_BULK, 40, False, 0)
    for r in (0, 1):
        lat = P.c.lat_get(r)
        assert P.c.lat_raw(r) == []
        assert lat["count"] == 40 and sum(lat["hist"]) == 40
        assert 0 < lat["min_ticks"] <= lat["max_ticks"] <= lat["sum_ticks"]


def test_accumulate_reset_disable(pair):
    P = pair
    want = untraced(P, mpx.MODE_PINGPONG, B_LL, 50, False)
    traced(P, mpx.MODE_PINGPONG, B_LL, 50, False, 64)
    first = {r: P.c.lat_get(r) for r in (0, 1)}
    out, errs = P.run(mpx.MODE_PINGPONG, B_LL, 50)
    assert not errs, errs
    for r in (0, 1):
        lat, raw = P.c.lat_get(r), P.c.lat_raw(r)
        assert lat["count"] == 100 and lat["calls"] == 2 and lat["last_iters"] == 50 and sum(lat["hist"]) == 100
        d = [b - a for a, b in zip(raw, raw[1:])]                # the second call's
        assert len(raw) == 51
        assert lat["sum_ticks"] == first[r]["sum_ticks"] + sum(d)
        assert lat["min_ticks"] == min(first[r]["min_ticks"], min(d))
        assert lat["max_ticks"] == max(first[r]["max_ticks"], max(d))
        assert lat["hist"] == [a + b for a, b in zip(first[r]["hist"], bucket_counts(d))]
        assert lat["max_iter"] == (int(np.argmax(d)) if max(d) > first[r]["max_ticks"] else first[r]["max_iter"])
        P.c.lat_reset(r)
        z = P.c.lat_get(r)
        assert all(z[k] == 0 for k in ("count", "calls", "min_ticks", "max_ticks", "sum_ticks", "max_iter",
                                        "last_iters")) and not any(z["hist"])
        assert P.c.lat_raw(r) == []
    for r in (0, 1):
        P.c.lat_disable(r)
        for call in (P.c.lat_get, P.c.lat_raw, P.c.lat_reset):
            with pytest.raises(mpx.MpxError) as e:
                call(r)
            assert e.value.status == mpx.ERR_STATE
    out, errs = P.run(mpx.MODE_PINGPONG, B_LL, 50)
    assert not errs, errs
    for r in (0, 1):
        assert {f: getattr(out[r], f) for f in RESULT_FIELDS} == want[r]


def test_enabling_again_with_a_larger_cap_regrows():
    """a context of its own, so that the block is first allocated for cap 4:
    cap 64 takes a new block (the old one retires), and enable clears"""
    P = Pairs("kernel", 1, B_LL)
    try:
        for cap in (4, 64):
            for r in (0, 1):
                P.c.lat_enable(r, cap)
            out, errs = P.run(mpx.MODE_PINGPONG, B_LL, 6)
            assert not errs, errs
            if cap == 4:
                assert all(len(P.c.lat_raw(r)) == 5 for r in (0, 1))
        for r in (0, 1):
            raw, lat = P.c.lat_raw(r), P.c.lat_get(r)
            assert len(raw) == 7
            assert lat["count"] == 6 and lat["calls"] == 1 and lat["last_iters"] == 6 and sum(lat["hist"]) == 6
            assert lat["sum_ticks"] == raw[-1] - raw[0] == sum(b - a for a, b in zip(raw, raw[1:]))
            assert out[r].check_failures == 0 and out[r].check_iters == 6
    finally:
        P.close()


def test_a_stalled_iteration_is_attributed_to_its_index(pair, monkeypatch):
    """positive control: rank 1's last workgroup stalls 20 ms before pulling
    the call's last payload (MPX_TEST lag_wg), so iteration 19 of 20 — and only
    it — takes >= 20 ms on both sides: rank 1's workgroup 0 waits for that
    chunk before its send, rank 0 waits for that send.  The stall is sized
    in ticks by the library (us x 100), so the tick count alone would pass
    at any clock rate: the host's own clock must have seen the 20 ms too
    (less the 2 % of test_kernel_clock_against_events_and_the_host_clock)."""
    P = pair
    monkeypatch.setenv("MPX_TEST", "lag_wg=1:-1:20000")
    out = traced(P, mpx.MODE_PINGPONG, B_BULK, 20, True, 64)
    monkeypatch.setenv("MPX_TEST", "")
    for r in (0, 1):
        print(f"rank {r}: wall_s {out[r].wall_s:.6f} device_s {out[r].device_s:.6f}")
        assert out[r].wall_s >= 0.0196
        lat, raw = P.c.lat_get(r), P.c.lat_raw(r)
        print(f"rank {r}: max {lat['max_ticks']} ticks at iteration {lat['max_iter']}, "
              f"p50 {mpx.lat_quantile(lat, 0.5)}, deltas {[b - a for a, b in zip(raw, raw[1:])]}")
        assert lat["count"] == 20
        assert lat["max_iter"] == 19
        assert lat["max_ticks"] >= 2_000_000
        assert mpx.lat_quantile(lat, 0.5) < lat["max_ticks"]
        assert mpx.lat_quantile(lat, 1.0) == mpx.lat_bucket_floor(mpx.lat_bucket(lat["max_ticks"]))


CLOCK_ITERS = 30000
# t[iters], the recorder's last tick, is read inside the loop, the kTsLoop stamp
# right after it: the tick's histogram add and raw store and a second clock
# read lie between.  Measured 20 to 40 ticks (the clock steps by 4) over 16
# calls of 1 to 30000 iterations on both ranks; allowed ten
# times the largest
GAP_MEASURED_TICKS = 40
GAP_S = 10 * GAP_MEASURED_TICKS * TICK


def test_kernel_clock_against_events_and_the_host_clock(pair):
    """Every kernel-side time is ticks x 1e-8 s (complete_call, mpx_lat.tick_s,
    the lag knob, the go timeout).  One unarmed 8-byte ping-pong long enough
    that dispatch and completion (tens of microseconds) are under 0.5 % of
    it: the kernel's span by its own clock must lie inside the hipEvent
    bracket of the same kernel and inside the host's CLOCK_MONOTONIC span
    from the launch, and fill at least 98 % of each — two clocks the project
    does not scale.  A wrong rate constant is off by a factor of 2 or more.
    The recorder's figures of the same call tie mpx_lat.tick_s to the same
    scale: its iterations add up to the kernel's span less the wait for the
    peer's post and the tail, up to the instructions between the last tick
    and the kTsLoop stamp."""
    P = pair
    out = traced(P, mpx.MODE_PINGPONG, B_LL, CLOCK_ITERS, False, 0, check=False)
    for r in (0, 1):
        t, ph, lat = out[r], P.c.phases(r), P.c.lat_get(r)
        P.c.lat_disable(r)
        k = ph["kernel_s"]
        print(f"rank {r}: kernel_s {k:.6f} device_s {t.device_s:.6f} wall_s {t.wall_s:.6f} "
              f"kernel/device {k / t.device_s:.5f} kernel/wall {k / t.wall_s:.5f}")
        assert ph["armed"] == 0 and t.wall_s == ph["wall_s"]
        assert t.device_s >= 0.020, "too short for the 2 % bound: raise CLOCK_ITERS"
        assert k <= t.device_s and k <= t.wall_s
        assert k >= 0.98 * t.device_s
        assert k >= 0.98 * t.wall_s
        loop_s = k - ph["posted_wait_s"] - ph["tail_s"]
        gap = loop_s - lat["sum_ticks"] * lat["tick_s"]
        print(f"rank {r}: loop {loop_s:.9f} s, recorded {lat['sum_ticks']} ticks, gap {gap / TICK:.2f} ticks")
        assert lat["count"] == CLOCK_ITERS
        assert -0.5 * TICK <= gap <= GAP_S + 0.5 * TICK


def test_other_engines_refuse_the_recorder():
    with mpx.Context(2, "sdma") as c:
        with pytest.raises(mpx.MpxError) as e:
            c.lat_enable(0, 16)
        assert e.value.status == mpx.ERR_UNSUPPORTED


def test_nonblocking_calls_run_untraced(pair):
    P = pair
    for pull in (False, True):
        want = untraced(P, mpx.MODE_NONBLOCKING, B_BULK, 30, pull)
        out = traced(P, mpx.MODE_NONBLOCKING, B_BULK, 30, pull, 64)
        for r in (0, 1):
            assert {f: getattr(out[r], f) for f in RESULT_FIELDS} == want[r]
            lat = P.c.lat_get(r)
            assert lat["calls"] == 0 and lat["count"] == 0 and P.c.lat_raw(r) == []


def test_recorder_and_armed_calls(pair):
    P = pair
    c = P.c
    for r in (0, 1):
        c.lat_disable(r)
    exp = P.expect(0, B_LL)
    args = (mpx.MODE_PINGPONG, 1, 0, 1, 10, P.bufs[0][0], P.bufs[0][1], B_LL)
    kw = dict(check_payload=True, expect=exp[0], expect_ack=exp[1], timeout_ms=10000)
    c.arm(*args, **kw)
    try:
        for call in (lambda: c.lat_enable(0, 16), lambda: c.lat_disable(0)):
            with pytest.raises(mpx.MpxError) as e:
                call()
            assert e.value.status == mpx.ERR_STATE
    finally:
        c.disarm(0)
    # enable, then arm, then start: the armed call is traced
    want = untraced(P, mpx.MODE_UNIDIR, B_BULK, 25, False)
    out = traced(P, mpx.MODE_UNIDIR, B_BULK, 25, False, 64, armed=True)
    for r in (0, 1):
        lat, raw = c.lat_get(r), c.lat_raw(r)
        d = [b - a for a, b in zip(raw, raw[1:])]
        assert lat["count"] == 25 and lat["calls"] == 1 and len(raw) == 26
        assert (lat["min_ticks"], lat["max_ticks"], lat["sum_ticks"]) == (min(d), max(d), sum(d))
        assert {f: getattr(out[r], f) for f in RESULT_FIELDS} == want[r]
        assert c.phases(r)["armed"] == 1
        c.lat_disable(r)


# ---- mpx_perf -L ------------------------------------------------------------
LAT_HEADER = ("Timestamp,JobId,Rank,PeerRank,Mode,BufferSize,NumOfBuffers,RunId,Count,MinUs,P50Us,P90Us,P99Us,P999Us,"
              "MaxUs,MeanUs,MaxIter")


def run_perf(tmp, args):
    tmp.mkdir()
    g1 = tmp / "group1"
    g1.write_text("vm\n")
    logs = tmp / "logs"
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", MPX_TEST="")
    p = run_bounded([PERF, "-g", "0,0", "-t", "5000", "-w", "2", "-f", str(g1), "-n", "1", "-p", "1", "-l", str(logs)]
                    + args, env=env)
    assert p.returncode == 0, p.stderr[-600:]
    recs = []
    for f in sorted(glob.glob(str(logs / "tcp-*.log"))):
        recs += [line.rstrip("\n").split(",") for line in open(f)]
    # a record with its timestamp, job id and time masked (mpi_perf.c:551)
    masked = sorted(",".join(["T", "U"] + f[2:9] + ["X", f[10]]) for f in recs)
    side = sorted(glob.glob(str(logs / "gpu-*.csv")))
    return masked, side, sorted(os.listdir(logs))


@pytest.mark.parametrize("unidir", [[], ["-u", "1"]])
def test_mpx_perf_writes_the_latency_side_file(tmp_path, unidir):
    args = ["-r", "3", "-i", "50", "-b", "8"] + unidir
    plain, plain_side, plain_files = run_perf(tmp_path / "plain", args)
    assert len(plain) == 2 and not [f for f in plain_files if f.startswith("lat-")]
    masked, side, files = run_perf(tmp_path / "lat", args + ["-L", "64"])
    assert masked == plain                                      # the records do not change
    assert len(side) == len(plain_side) == 1
    assert [len(open(f).readlines()) for f in side] == [len(open(f).readlines()) for f in plain_side]
    lat_files = [f for f in files if f.startswith("lat-")]
    assert len(lat_files) == 1 and len(files) == len(plain_files) + 1
    m = re.fullmatch(r"lat-([0-9a-f-]{36})-0-\d{4}-\d\d-\d\d-\d\d-\d\d-\d\d\.csv", lat_files[0])
    assert m, lat_files
    assert not fnmatch.fnmatch(lat_files[0], "tcp*") and not fnmatch.fnmatch(lat_files[0], "gpu-*.csv")
    lines = open(tmp_path / "lat" / "logs" / lat_files[0]).read().splitlines()
    assert lines[0] == LAT_HEADER
    rows = [dict(zip(LAT_HEADER.split(","), x.split(","))) for x in lines[1:]]
    assert [int(x["RunId"]) for x in rows] == [1, 2]            # one line per recorded run
    for x in rows:
        assert x["JobId"] == m.group(1) and (x["Rank"], x["PeerRank"]) == ("0", "1")
        assert int(x["Mode"]) == (mpx.MODE_UNIDIR if unidir else mpx.MODE_PINGPONG)
        assert (int(x["BufferSize"]), int(x["NumOfBuffers"]), int(x["Count"])) == (8, 50, 50)
        mn, p50, p90, p99, p999, mx = (float(x[k]) for k in ("MinUs", "P50Us", "P90Us", "P99Us", "P999Us", "MaxUs"))
        assert 0 < mn <= p50 <= p90 <= p99 <= p999 <= mx
        assert mn <= float(x["MeanUs"]) <= mx and 0 <= int(x["MaxIter"]) < 50
