"""mpx_xfer_fan: one rank exchanges a block with every one of its peers in one
launch (-m gpu, MI355X).

Loopback ranks on GPU 0, one host thread per rank (tests/fan.py).  Every
expectation is host bytes: tx is written from the host with distinct seeded
bytes per (src, dst), rx is 0xEE before a call and read back WHOLE after it
(so the gaps between blocks, the rank's own block and the blocks of ranks
outside the peer set must still be 0xEE), tx is read back unchanged, and the
digests are recomputed on the host (oracle_py).  3 iterations unless stated.
"""
import json
import os
import subprocess
import sys

import pytest

import mpx
import oracle_py as O
import payload
from fan import M64, Fan, fan_width, full_mesh, round16
from payload import chunk_shape

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PINGPONG, NONBLOCKING, UNIDIR = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING, mpx.MODE_UNIDIR
ITERS = 3
N = 65555                      # five workgroups per link by the default rule, a ragged tail

RING4 = {0: [1, 3], 1: [2, 0], 2: [3, 1], 3: [0, 2]}       # each rank lists its two neighbours in another order
STAR4 = {0: [3, 1, 2], 1: [0], 2: [0], 3: [0]}
SHAPES = {"pair": (2, full_mesh(2)), "mesh3": (3, full_mesh(3)), "mesh4": (4, full_mesh(4)), "ring4": (4, RING4),
          "star4": (4, STAR4)}


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(shape, check):
    """K = 1, an odd world, a full mesh of 4, a ring whose two untouched
    blocks stay 0xEE, and a star whose hub has three links and whose leaves
    one: the width depends only on what both ends see, so both sides of every
    link report the same one"""
    n, sets = SHAPES[shape]
    F = Fan(n, n * round16(N) + payload.GUARD)
    try:
        F.layout(N, round16(N))
        out, errs = F.run(sets, ITERS, check=check)
        assert not errs, errs
        width = fan_width(n, N)
        assert width == mpx.fan_width(n, N) == 5
        F.verify(sets, out, ITERS, check, (shape, check), widths=width)
    finally:
        F.close()


SIZES = [0, 1, 15, 16, 17, 4097, 65555, 456131]


@pytest.mark.parametrize("stream", [False, True])
@pytest.mark.parametrize("check", [True, False])
def test_sizes_and_iteration_counts(check, stream):
    """block lengths around the 16-byte unit, the 1 KiB narrowing and the
    chunk size, at stride = the length rounded up to 16 and once at 4096, for
    1, 2 and 5 iterations, plain and streaming stores; three ranks, full mesh"""
    sets = full_mesh(3)
    F = Fan(3, 3 * round16(max(SIZES)) + payload.GUARD)
    try:
        for n in SIZES:
            for stride in [round16(n)] + ([4096] if n == 17 else []):
                F.layout(n, stride)
                for iters in (1, 2, 5):
                    what = (n, stride, iters, check, stream)
                    out, errs = F.run(sets, iters, check=check, stream=stream)
                    assert not errs, (what, errs)
                    F.verify(sets, out, iters, check, what, widths=fan_width(3, n))
    finally:
        F.close()


EDGE_NWG, EDGE_N = 96, 98305


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("check", [True, False])
def test_chunk_edges(check, nranks):
    """explicit width 96 at 98305 bytes: chunks of 1040 bytes, workgroup 95
    empty (it moves nothing and must still publish, credit and count),
    workgroup 94 holding 545 bytes (34 units and a 1-byte tail); at 3 ranks
    3 x 2 x 96 = 576 workgroups share the GPU"""
    assert chunk_shape(EDGE_NWG, EDGE_N) == (96, 1040, 1, 94, 545) and 545 % 16 == 1
    assert 95 * 1040 >= EDGE_N > 94 * 1040
    sets = full_mesh(nranks)
    F = Fan(nranks, nranks * round16(EDGE_N) + payload.GUARD)
    try:
        F.layout(EDGE_N, round16(EDGE_N))
        out, errs = F.run(sets, ITERS, check=check, nwg=EDGE_NWG)
        assert not errs, errs
        F.verify(sets, out, ITERS, check, ("edges", nranks, check), widths=96)
        assert all(out[r][0].nwg == 96 for r in sets)
    finally:
        F.close()


def test_accounting_and_link_counters():
    """per link, tx_seq and rx_seq grow by iters and calls by one (none for
    iters = 0); the rank's token by one per call; a link outside the peer set
    does not move"""
    F = Fan(4, 4 * round16(N) + payload.GUARD)
    try:
        F.layout(N, round16(N))
        for sets, iters, check in ((full_mesh(4), 4, True), (RING4, 0, False), (STAR4, 2, False), (RING4, 7, True)):
            before = {(r, p): F.counters(r, p) for r in range(4) for p in range(4) if p != r}
            out, errs = F.run(sets, iters, check=check)
            assert not errs, errs
            F.verify(sets, out, iters, check, ("counters", iters))
            for (r, p), b in before.items():
                a = F.counters(r, p)
                on = p in sets.get(r, [])
                assert a["tx_seq"] == b["tx_seq"] + (iters if on else 0), (r, p, b, a)
                assert a["rx_seq"] == b["rx_seq"] + (iters if on else 0), (r, p, b, a)
                assert a["calls"] == b["calls"] + (1 if on and iters > 0 else 0), (r, p, b, a)
                assert a["token"] == b["token"] + (1 if r in sets else 0), (r, p, b, a)
    finally:
        F.close()


def _pair_call(F, mode, n, iters, check):
    """an ordinary pair call between ranks 0 and 1 on the fan's buffers (the
    first n bytes of tx and rx), its payloads checked from host bytes"""
    import threading
    F.prefill()
    out, errs = {}, {}

    def side(r):
        h = F.host[1 - r]
        try:
            out[r] = F.c.xfer(mode, 1 if r == 0 else 0, r, 1 - r, iters, F.bufs[r][0], F.bufs[r][1], n,
                              check_payload=check, expect=O.checksum(h[:n]), expect_ack=O.checksum(h[:1]),
                              timeout_ms=5000)
        except mpx.MpxError as e:
            errs[r] = e

    th = [threading.Thread(target=side, args=(r,)) for r in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, (mode, errs)
    for r in (0, 1):
        m = 1 if (mode == UNIDIR and r == 0) else n
        assert out[r].check_failures == 0 and out[r].check_iters == (iters if check else 0), (mode, r)
        payload.assert_region(F.c, F.bufs[r][1], 0, F.host[1 - r][:m], what=f"pair call mode {mode}: rx of rank {r}")
        payload.compare(F.c.read(F.bufs[r][0], F.cap), F.host[r], 0, f"pair call mode {mode}: tx of rank {r}")


def test_interleaved_with_pair_calls_on_the_same_links():
    """ping-pong -> fan -> unidir -> fan (checked) -> non-blocking checked ->
    fan on the links of one context: every call passes with its payloads
    checked, so each fan call left the rank's scratch words zero, the link
    counters and the posted / flag / credit words where a pair call expects
    them, and each pair call left them where a fan call does"""
    n = 20001
    sets = full_mesh(3)
    F = Fan(3, 3 * round16(n) + payload.GUARD)
    try:
        F.layout(n, round16(n))
        _pair_call(F, PINGPONG, n, 4, True)
        out, errs = F.run(sets, ITERS, check=False)
        assert not errs, errs
        F.verify(sets, out, ITERS, False, "fan after ping-pong")
        _pair_call(F, UNIDIR, n, 4, True)
        out, errs = F.run(sets, ITERS, check=True)
        assert not errs, errs
        F.verify(sets, out, ITERS, True, "fan after unidir")
        _pair_call(F, NONBLOCKING, n, 5, True)
        out, errs = F.run(sets, ITERS, check=True, stream=True)
        assert not errs, errs
        F.verify(sets, out, ITERS, True, "fan after non-blocking")
        _pair_call(F, PINGPONG, 8, 3, True)       # an LL message after a fan call
    finally:
        F.close()


def test_lost_payload_is_caught(monkeypatch):
    """Negative control (MPX_TEST=skip_push=2: push 2 of every link moves no
    payload, its flag still goes).  Checked, the call returns MPX_ERR_CHECK
    with a failure on every link: receive 2 reads the poison left on receive
    1.  Unchecked the call succeeds, and so must the byte comparison: every
    push of a call carries the same bytes, and push 1 delivered them.  A lost
    payload shows in the bytes only when no other push carries them, so the
    unchecked control is skip_push=1 on a one-iteration call: the call
    succeeds, rx keeps its prefill, and the host byte comparison raises."""
    monkeypatch.setenv("MPX_TEST", "skip_push=2")
    sets = full_mesh(3)
    F = Fan(3, 3 * round16(N) + payload.GUARD)
    try:
        F.layout(N, round16(N))
        out, errs = F.run(sets, ITERS, check=True)
        assert not out and sorted(errs) == [0, 1, 2], (out, errs)
        for r, e in errs.items():
            assert e.status == mpx.ERR_CHECK, (r, e)
            assert e.timing.check_failures >= 2 and e.timing.check_iters == 2 * ITERS, r
            assert len(e.links) == 2 and all(l["check_failures"] >= 1 for l in e.links), (r, e.links)
        out, errs = F.run(sets, ITERS, check=False)
        assert not errs, errs
        F.verify(sets, out, ITERS, False, "push 2 lost, pushes 1 and 3 delivered")
        monkeypatch.setenv("MPX_TEST", "skip_push=1")
        out, errs = F.run(sets, 1, check=False)
        assert not errs, errs
        F.verify_bytes(sets, "the only push lost: rx keeps its prefill", moved=False)
        with pytest.raises(AssertionError, match="bytes differ, first at offset"):
            F.verify_bytes(sets, "lost payload")
        monkeypatch.setenv("MPX_TEST", "")
        out, errs = F.run(sets, ITERS, check=True)
        assert not errs, errs
        F.verify(sets, out, ITERS, True, "after the knob")
    finally:
        F.close()


def _status(F, r, peers, block_len=None, stride=None, **kw):
    try:
        F.c.fan(r, peers, ITERS, F.bufs[r][0], F.bufs[r][1], F.block_len if block_len is None else block_len,
                F.stride if stride is None else stride, timeout_ms=2000, **kw)
    except mpx.MpxError as e:
        return e.status
    return mpx.OK


def test_refusals_leave_the_rank_usable(monkeypatch):
    """every refusal returns its status before any GPU work (the peers do not
    call), takes no number from the links, and a valid call follows"""
    sets = full_mesh(3)
    big = 262144
    F = Fan(3, 3 * big + payload.GUARD)
    try:
        F.layout(N, round16(N))
        before = {(r, p): F.counters(r, p) for r in range(3) for p in range(3) if p != r}
        assert _status(F, 0, [1, 1]) == mpx.ERR_INVALID                      # a duplicate peer
        assert _status(F, 0, [1, 0]) == mpx.ERR_INVALID                      # itself
        assert _status(F, 0, [1, 3]) == mpx.ERR_INVALID                      # a rank the context does not have
        assert _status(F, 0, []) == mpx.ERR_INVALID
        assert _status(F, 0, [1, 2], stride=round16(N) + 8) == mpx.ERR_INVALID   # stride % 16
        assert _status(F, 0, [1, 2], stride=round16(N) - 16) == mpx.ERR_INVALID  # stride < block_len
        assert _status(F, 0, [1, 2], block_len=big, stride=big + 4096) == mpx.ERR_INVALID   # block 2 past the length
        assert _status(F, 0, [1, 2], block_len=big, stride=big, nwg=200) == mpx.ERR_INVALID  # 400 workgroups
        assert _status(F, 0, [1, 2], nwg=257) == mpx.ERR_INVALID
        # a call that fails after taking its numbers and before its launch gives them back
        monkeypatch.setenv("MPX_TEST", "fail_launch=0")
        assert _status(F, 0, [1, 2]) == mpx.ERR_HIP
        monkeypatch.setenv("MPX_TEST", "")
        assert before == {k: F.counters(*k) for k in before}
        F.c.arm(PINGPONG, 1, 0, 1, 2, F.bufs[0][0], F.bufs[0][1], 4097, timeout_ms=2000)
        armed = F.counters(0, 1)
        assert _status(F, 0, [1, 2]) == mpx.ERR_STATE                        # holds an armed call
        assert F.counters(0, 1) == armed
        F.c.disarm(0)
        out, errs = F.run(sets, ITERS, check=True)
        assert not errs, errs
        F.verify(sets, out, ITERS, True, "after the refusals")
    finally:
        F.close()
    S = Fan(2, 2 * round16(N) + payload.GUARD, engine="sdma")
    try:
        S.block_len, S.stride = N, round16(N)
        assert _status(S, 0, [1]) == mpx.ERR_UNSUPPORTED
    finally:
        S.close()


def test_timeout_when_the_peer_never_calls():
    """the kernel's bounded exit (modelled on test_timeout_when_peer_never_runs):
    rank 0 waits 300 ms for a post that never comes, the call returns
    MPX_ERR_TIMEOUT, and the rank refuses further calls"""
    F = Fan(2, 2 * round16(N) + payload.GUARD)
    try:
        F.layout(N, round16(N))
        out, errs = F.run({0: [1]}, ITERS, check=True, timeout_ms=300)
        assert 0 in errs and errs[0].status == mpx.ERR_TIMEOUT, (out, errs)
        out, errs = F.run({0: [1]}, 1, check=False, timeout_ms=300, prefill=False)
        assert errs[0].status == mpx.ERR_STATE
    finally:
        F.close()


def test_two_processes_full_mesh(tmp_path):
    """two processes with two ranks each (tests/fan_worker.py): every rank's
    three links, two of them over imported ranks, checked"""
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "fan_worker.py"), str(tmp_path), str(p)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for p in (0, 1)]
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
            assert x["rx_ok"] and x["tx_ok"], x
            assert x["check_failures"] == 0 and x["check_iters"] == 3 * x["iters"] and x["recv_done"] == 3 * x["iters"], x
            assert x["protocol"] == 9 and x["digest_ok"], x
            assert [l["recv_done"] for l in x["links"]] == [x["iters"]] * 3, x


# ---- the host front end: mpx_perf -m 1 --------------------------------------
FAN_ARGS = ["-m", "1", "-c", "2", "-r", "3", "-i", "5", "-b", "65555", "-f", "@G1", "-n", "1", "-p", "1", "-l", "@LOGS"]


def _check_fan_run(recs, side):
    """3 ranks x 2 recorded runs (run 0 is dropped, mpi_perf.c:545): VMCount =
    world, NumOfFlows = world - 1, LocalIP = RemoteIP; 6 link lines per run in
    gpu-*.csv, protocol fan, every payload checked, none failed"""
    assert len(recs) == 3 * 2, recs
    assert sorted((int(f[2]), int(f[10])) for f in recs) == [(r, run) for r in range(3) for run in (1, 2)]
    for f in recs:
        assert len(f) == 11 and int(f[3]) == 3 and int(f[6]) == 2 and f[4] == f[5] == "127.0.0.1", f
        assert int(f[7]) == 65555 and int(f[8]) == 5, f
    assert len(side) == 2 * 6, side
    for run_id in (1, 2):
        lines = [f for f in side if int(f[17]) == run_id]
        assert sorted((int(f[2]), int(f[6])) for f in lines) == [(r, p) for r in range(3) for p in range(3) if p != r]
    width = fan_width(3, 65555)
    for f in side:
        assert f[3] == "kernel" and f[13] == "fan" and int(f[14]) == width == 5, f
        assert int(f[8]) == 65555 and int(f[9]) == 5 and int(f[15]) == 5 and int(f[16]) == 0, f
        assert int(f[18]) == 5 and float(f[11]) >= 0, f
        # -c 2: block (src = PeerRank, dst = Rank) of that run, five times
        want = O.pattern_checksum(65555, mpx.FILL_SPLITMIX,
                                  mpx.pattern_key(mpx.PATTERN_SEED, int(f[6]), int(f[2]), int(f[17])))
        assert int(f[19]) == (5 * want) & M64, f


def test_mpx_perf_fan_threads_mode(tmp_path):
    from test_gpu_host import run
    p, recs, side = run(tmp_path, ["-w", "3"] + FAN_ARGS, names="vm,runsc,runsc", gpus="0,0,0")
    assert p.returncode == 0, p.stderr[-800:]
    assert "FAN: each of 3 ranks" in p.stderr
    _check_fan_run(recs, side)


def test_mpx_perf_fan_processes_mode(tmp_path):
    from test_gpu_host import run_procs
    rcs, err, recs, side = run_procs(tmp_path, FAN_ARGS, 3, "vm,runsc,runsc")
    assert rcs == [0, 0, 0], err[-800:]
    assert len({f[1] for f in recs}) == 1             # one JobId
    _check_fan_run(recs, side)
