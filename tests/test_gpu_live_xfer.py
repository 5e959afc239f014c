"""Mid-call probes of the pair and fan loops (tests/probe.py; -m gpu).

Outside check mode — the mode every timed run uses — nothing in the suite sees
a loop's iterations between its first and its last: every push writes the same
tx into the same rx.  Here loopback ranks on GPU 0 run one long call each, on
threads of their own (tests/pairs.py, tests/fan.py), and the test thread
watches their receive buffers through the context's utility stream, which
runs beside the ranks' kernels: mpx_fill overwrites the WHOLE attached rx with
0xEE (rx is attached 4 KiB longer than the message, so the rest is guard),
mpx_read polls it until every payload byte is back and every other byte is
still 0xEE.  tx is never touched (read-only during a call; the staged push
reads it once per call); no kernel reads rx payload outside check mode, and
the next push rewrites it.

A counted probe proves that the loop rewrote every byte after the poison, at
>= 8 distinct times through the call; how many pushes a call made stays
pinned by recv_done and the link counters.
"""
import numpy as np
import pytest

import mpx
import oracle_py as O
import payload
import probe
from fan import Fan, full_mesh
from fan_ll import LLFan
from pairs import Pairs

pytestmark = pytest.mark.gpu

POISON = payload.GUARD_BYTE
ROOM = 4096                       # rx is attached this much longer than buff_len
DEADLINES = dict(start_deadline_s=2.0, probe_deadline_s=2.0, join_deadline_s=60.0)
PINGPONG, NONBLOCKING, UNIDIR = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING, mpx.MODE_UNIDIR
MODE_NAMES = {PINGPONG: "pingpong", NONBLOCKING: "nonblocking", UNIDIR: "unidir"}
STAGED = (256 << 10) + 16 + 5     # LDS-staged at the default width
LL_LOOPBACK_MAX = 2048            # loopback links switch from LL to bulk above 2 KiB


class RxSurface:
    """the first `length` bytes of a rank's rx (all that is attached), seen
    through the utility stream.  parts: [(offset, bytes)] the loop writes;
    everything else must stay 0xEE."""

    def __init__(self, ctx, rx, length: int, parts):
        self.ctx, self.rx, self.length, self.poison_byte = ctx, rx, length, POISON
        self.expected = np.full(length, POISON, np.uint8)
        self.guards = np.ones(length, bool)
        for off, data in parts:
            assert 0 <= off and off + len(data) <= length
            self.expected[off:off + len(data)] = np.frombuffer(bytes(data), np.uint8)
            self.guards[off:off + len(data)] = False

    def poison(self):
        self.ctx.fill(self.rx, self.length, mpx.FILL_BYTE, POISON)

    def snapshot(self):
        return np.frombuffer(self.ctx.read(self.rx, self.length), np.uint8)


def probed(request, capsys, what, surface, call, wall_of, verify):
    """the case's plan (module docstring of tests/probe.py): a 2000-iteration
    unprobed call for the byte check and the sizing, then the probed call;
    call(iters) -> the call's results, wall_of(results) -> seconds,
    verify(results, iters) asserts what the call reported"""
    surface.poison()
    out = call(probe.SIZING_ITERS)
    verify(out, probe.SIZING_ITERS)
    payload.compare(surface.snapshot().tobytes(), surface.expected.tobytes(), 0, f"{what}: rx after the sizing call")
    iters = probe.size_iters(wall_of(out))
    rep = probe.run_probed(lambda: call(iters), surface, poll_sleep_s=0.0, iters=iters, **DEADLINES)
    probe.say(request, capsys, f"{what}: {rep}; sizing call {wall_of(out) * 1e3:.2f} ms, probed call "
                                f"{wall_of(rep.result) * 1e3:.1f} ms")
    verify(rep.result, iters)
    probe.require(rep)


# ---- pairs ------------------------------------------------------------------------
def pair_case(request, capsys, engine, mode, n, proto, **kw):
    P = Pairs(engine, 1, n + ROOM, fill="pattern")
    try:
        tx = {r: O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, r, 0, 0)) for r in (0, 1)}
        # ping-pong and non-blocking: both ranks receive n bytes; unidir: rank 1
        # does, rank 0 (the sender) the 1-byte ack (mpi_perf.c:137,142)
        got = {r: 1 if (mode == UNIDIR and r == 0) else n for r in (0, 1)}
        surface = probe.Joined([(f"rank {r} rx", RxSurface(P.c, P.bufs[r][1], n + ROOM, [(0, tx[1 - r][:got[r]])]))
                                for r in (0, 1)])

        def call(iters):
            out, errs = P.run(mode, n, iters, check=False, timeout_ms=0, **kw)
            assert not errs, errs
            return out

        def verify(out, iters):
            done = O.lib().oracle_nb_waited(iters) if mode == NONBLOCKING else iters
            for r in (0, 1):
                t = out[r]
                assert t.recv_done == done and t.check_iters == 0 and t.check_failures == 0, (r, t.as_dict())
                assert t.bytes == n * iters * (1 if mode == UNIDIR else 2), (r, t.as_dict())
                if mode != UNIDIR or r == 0 or proto not in ("ll", "bulk"):   # (a push: the side that moves payload)
                    assert mpx.PROTOCOLS[t.protocol] == proto, (r, t.as_dict())
                    if kw.get("nwg") and proto == "bulk":
                        assert t.nwg == kw["nwg"], (r, t.as_dict())

        what = f"{engine} {MODE_NAMES[mode]} {n} B {kw or ''}"
        probed(request, capsys, what, surface, call, lambda out: max(out[r].wall_s for r in (0, 1)), verify)
    finally:
        P.close()


def kernel_proto(mode, n):
    return "ll" if (mode != NONBLOCKING and n <= LL_LOOPBACK_MAX) else "bulk"


@pytest.mark.parametrize("mode", [PINGPONG, NONBLOCKING, UNIDIR], ids=MODE_NAMES.get)
@pytest.mark.parametrize("n", [8, 2045, 4161, STAGED])
def test_pair_loop_keeps_delivering(request, capsys, mode, n):
    """8 B and 2045 B: LL (ping-pong, unidir); 4161 B: the first bulk size,
    ragged tail; 256 KiB + 21: 17 workgroups pushing from LDS"""
    pair_case(request, capsys, "kernel", mode, n, kernel_proto(mode, n))


@pytest.mark.parametrize("mode", [PINGPONG, NONBLOCKING, UNIDIR], ids=MODE_NAMES.get)
@pytest.mark.parametrize("kw", [dict(stage=False), dict(stream=True), dict(nwg=7)], ids=["nostage", "stream", "width7"])
def test_staged_size_other_push_forms(request, capsys, mode, kw):
    """256 KiB + 21 pushed from memory every time (MPX_XFER_NOSTAGE), with the
    streaming store hint (MPX_XFER_STREAM), and at an explicit width (7:
    chunks of 37456 B, the last one ragged, 37429 B)"""
    pair_case(request, capsys, "kernel", mode, STAGED, "bulk", **kw)


def test_width_that_leaves_an_empty_chunk(request, capsys):
    """(70, 71681) of payload.EDGE_CASES: 1040-byte chunks, workgroup 69's is
    empty and workgroup 68's has 961 bytes"""
    assert payload.chunk_shape(70, 71681) == (70, 1040, 1, 68, 961)
    pair_case(request, capsys, "kernel", PINGPONG, 71681, "bulk", nwg=70)


@pytest.mark.parametrize("mode", [PINGPONG, UNIDIR], ids=MODE_NAMES.get)
@pytest.mark.parametrize("n", [4161, (256 << 10) + 21])
def test_pull_loop_keeps_delivering(request, capsys, mode, n):
    pair_case(request, capsys, "kernel", mode, n, "pull", pull=True)


@pytest.mark.parametrize("mode", [PINGPONG, UNIDIR], ids=MODE_NAMES.get)
@pytest.mark.parametrize("pull", [False, True], ids=["push", "pull"])
def test_sdma_loop_keeps_delivering(request, capsys, mode, pull):
    """the SDMA engine's graph-captured 256-iteration chunks and their remainder"""
    pair_case(request, capsys, "sdma", mode, 4161, "sdma_pull" if pull else "sdma", pull=pull)


@pytest.mark.parametrize("n", [4161, STAGED])
def test_self_send_keeps_delivering(request, capsys, n):
    """the non-blocking loop of a rank paired with itself: one launch, one stream"""
    c = mpx.Context(1, "kernel")
    try:
        tx, rx = c.alloc(0, n + ROOM), c.alloc(0, n + ROOM)
        key = mpx.pattern_key(mpx.PATTERN_SEED, 0, 0, 7)
        c.fill(tx, n + ROOM, mpx.FILL_SPLITMIX, key)
        c.attach(0, 0, tx, rx, n + ROOM)
        surface = RxSurface(c, rx, n + ROOM, [(0, O.fill(n, mpx.FILL_SPLITMIX, key))])

        def verify(t, iters):
            assert (t.recv_done, t.bytes, t.check_iters) == (O.lib().oracle_nb_waited(iters), 2 * n * iters, 0), \
                t.as_dict()
            assert mpx.PROTOCOLS[t.protocol] == "bulk", t.as_dict()

        probed(request, capsys, f"self-send {n} B", surface,
               lambda iters: c.xfer(NONBLOCKING, 0, 0, 0, iters, tx, rx, n), lambda t: t.wall_s, verify)
    finally:
        c.close()


# ---- fan --------------------------------------------------------------------------
def fan_case(request, capsys, F, block_len, stride, proto, **kw):
    """ranks 0, 1, 2 of F's four exchange in a full mesh; rank 3 is attached
    and outside the set.  In every rx the peers' blocks come back; the gaps
    between blocks, the rank's own block, rank 3's block and the room behind
    the last block stay 0xEE."""
    try:
        F.layout(block_len, stride)
        F.prefill()
        sets = full_mesh(3)
        surface = probe.Joined([(f"rank {r} rx", RxSurface(F.c, F.bufs[r][1], F.caps[r],
                                                           [(p * stride, F.block(p, r)) for p in sets[r]]))
                                for r in sets])
        for r in sets:
            assert (surface.parts[r][1].expected.tobytes() == F.expected_rx(r, sets[r]))

        def call(iters):
            out, errs = F.run(sets, iters, check=False, timeout_ms=0, prefill=False, **kw)
            assert not errs, errs
            return out

        def verify(out, iters):
            for r, peers in sets.items():
                t, links = out[r]
                assert (mpx.PROTOCOLS.get(t.protocol, t.protocol), t.launches) == (proto, 1), (r, t.as_dict())
                assert t.bytes == 2 * block_len * iters * len(peers) and t.recv_done == len(peers) * iters, \
                    (r, t.as_dict())
                assert [l["peer"] for l in links] == peers and all(l["recv_done"] == iters for l in links), (r, links)

        what = f"{proto} block {block_len} B stride {stride}"
        probed(request, capsys, what, surface, call, lambda out: max(out[r][0].wall_s for r in sets), verify)
        payload.compare(F.c.read(F.bufs[3][1], F.caps[3]), bytes([POISON]) * F.caps[3], 0, f"{what}: rx of rank 3")
        for r in F.ranks:
            payload.compare(F.c.read(F.bufs[r][0], F.caps[r]), F.host[r], 0, f"{what}: tx of rank {r}")
    finally:
        F.close()


def test_bulk_fan_keeps_delivering(request, capsys):
    fan_case(request, capsys, Fan(4, 4 * 8192 + ROOM), 4161, 8192, "fan")


@pytest.mark.parametrize("n", [8, 4096])
def test_ll_fan_keeps_delivering(request, capsys, n):
    """MPX_FAN_LL at its smallest useful and its largest block"""
    stride = max(16, n)
    fan_case(request, capsys, LLFan(4, 4 * stride + ROOM), n, stride, mpx.PROTO_FAN_LL, ll=True)
