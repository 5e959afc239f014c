"""The host link's forced forms on the real kernel, check mode at the LL edges
and long calls (-m gpu).

MPX_HOSTLINK_LL is read at every call, so monkeypatch sets it per test:
0 makes every message with bytes a bulk message — the unidir 1-byte ack too,
pushed to the endpoint and pulled from it at the payload's width, so all
chunks but one are empty; 8192 makes 8 KiB LL messages, whose 2048 granules
workgroup 0 polls across the link.  Every expectation is host bytes
(tests/hostlink.py, LinkMap.call: the whole rx and tx of both ends, the
oracle's checksums, every counter of both ends); every wait is bounded.
"""
import pytest

import mpx
import payload
from hostlink import LinkMap

pytestmark = pytest.mark.gpu

PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
MODES = [PP, UNI]
GROUPS = [1, 0]
BIG = (256 << 10) + 21
LINK = (0, 1)

_maps = {}


def one(n: int) -> LinkMap:
    """GPU rank 0 and endpoint 1, built for messages of n bytes; shared by the cases of that size"""
    if n not in _maps:
        _maps[n] = LinkMap(n, 2, [0], [1], [LINK])
    return _maps[n]


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


@pytest.mark.parametrize("n,nwg", [(0, 0), (1, 0), (777, 0), (4161, 0), (71681, 70)])
@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_threshold_0_makes_everything_bulk(monkeypatch, mode, gpu_group, n, nwg):
    """MPX_HOSTLINK_LL=0: bulk on both sides whenever n > 0 (LinkMap.verify
    asserts PROTO_HOSTLINK_BULK), and 0 bytes stay LL (0 <= 0).  In unidir the
    ack is a 1-byte bulk message in the other direction: the payload's
    receiver holds exactly n bytes and the sender's rx exactly 1."""
    monkeypatch.setenv("MPX_HOSTLINK_LL", "0")
    assert mpx.hostlink_ll_max() == 0
    h = one(71681)
    out = h.call([LINK], mode, gpu_group, n, 5, nwg=nwg, what=("LL=0", mode, gpu_group, n))
    want = mpx.PROTO_HOSTLINK_BULK if n > 0 else mpx.PROTO_HOSTLINK_LL
    assert [t.protocol for t in out.values()] == [want, want]
    width = payload.chunk_shape(nwg if nwg else min(16, max(1, -(-n // 32768))), n)[0] if n > 0 else 1
    assert all(t.nwg == width for t in out.values()), [t.nwg for t in out.values()]
    if mode == UNI and n > 0:
        sender, receiver = (0, 1) if gpu_group == 1 else (1, 0)
        blank = h.blank()
        assert h.rx(sender)[:1] == h.tx_bytes[receiver][:1] and h.rx(sender)[1:] == blank[1:]
        assert h.rx(receiver)[:n] == h.tx_bytes[sender][:n] and h.rx(receiver)[n:] == blank[n:]


@pytest.mark.parametrize("n", [8185, 8192])
@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_threshold_8192_makes_8_kib_ll_messages(monkeypatch, mode, gpu_group, n):
    monkeypatch.setenv("MPX_HOSTLINK_LL", "8192")
    h = one(8192)
    out = h.call([LINK], mode, gpu_group, n, 5, what=("LL=8192", mode, gpu_group, n))
    assert all(t.protocol == mpx.PROTO_HOSTLINK_LL and t.nwg == 1 for t in out.values())
    assert h.c.phases(0)["kernel_s"] > 0      # (the GPU side ran its one-workgroup kernel)


@pytest.mark.parametrize("n", ["0", "1", "T", "T+1"])
@pytest.mark.parametrize("gpu_group", GROUPS)
@pytest.mark.parametrize("mode", MODES)
def test_check_mode_at_the_ll_edges(mode, gpu_group, n):
    """33 checked iterations at 0, 1, T and T + 1 bytes under the default
    threshold: every payload but the last is poisoned after its checksum, on
    whichever side received it"""
    T = mpx.hostlink_ll_max()
    n = {"0": 0, "1": 1, "T": T, "T+1": T + 1}[n]
    h = one(4161)
    h.call([LINK], mode, gpu_group, n, 33, what=("edges", mode, gpu_group, n))


@pytest.mark.parametrize("gpu_group,n", [(1, "8"), (1, "T+1"), (1, "4161"), (0, "4161")])
def test_a_long_call(gpu_group, n):
    """2049 checked ping-pong iterations — one past a power of two of the relay
    words (kScrHostSeen counts to 2049) and of kScrLanded, and ensure_csum
    grows: 8 B (LL), T + 1 B (bulk, one workgroup, no relay), 4161 B at five
    workgroups in both orientations.  (The default width at 4161 B is one
    workgroup — 32 KiB per workgroup — so the width is asked for: 16, which
    the 1 KiB-per-workgroup rule narrows to 5.)"""
    T = mpx.hostlink_ll_max()
    n = {"8": 8, "T+1": T + 1, "4161": 4161}[n]
    h = one(4161)
    out = h.call([LINK], PP, gpu_group, n, 2049, nwg=16 if n == 4161 else 0, what=("long", gpu_group, n))
    assert all(t.nwg == (5 if n == 4161 else 1) for t in out.values())


@pytest.mark.parametrize("n", [4161, BIG])
@pytest.mark.parametrize("mode", MODES)
def test_nostage(mode, n):
    """MPX_XFER_NOSTAGE: the GPU's bulk pushes read tx from memory every time"""
    h = one(BIG)
    h.call([LINK], mode, 1, n, 5, stage=False, what=("nostage", mode, n))
    if mode == PP:
        h.call([LINK], mode, 0, n, 5, stage=False, what=("nostage", mode, n, "the GPU answers"))


@pytest.mark.parametrize("args,h,n,iters", [(["-b", "8", "-c", "1", "-i", "7", "-r", "3"], "1", 8, 7),
                                            (["-b", "0", "-i", "3", "-r", "3"], "2", 0, 3)])
def test_mpx_perf_host_link_ll_runs(tmp_path, args, h, n, iters):
    """mpx_perf -H with LL sizes: -H 1 -b 8 -c 1 -i 7 -r 3 and -H 2 -b 0 -i 3;
    the side record names the protocol host_ll"""
    from test_gpu_host import run
    p, recs, side = run(tmp_path, ["-H", h, "-w", "1", "-f", "@G1", "-n", "1", "-p", "1", "-l", "@LOGS"] + args, gpus="0")
    assert p.returncode == 0, p.stderr[-600:]
    writer = 0 if h == "1" else 1
    assert len(recs) == 2 and len(side) == 2
    for f in recs:
        assert len(f) == 11 and int(f[7]) == n and int(f[8]) == iters
    for f in side:
        assert int(f[2]) == writer and int(f[6]) == 1 - writer and f[3] == "kernel" and f[13] == "host_ll"
        assert int(f[15]) == (iters if "-c" in args else 0) and int(f[16]) == 0 and int(f[18]) == iters
