"""Mid-call probes of the host link's loops (tests/probe.py; -m gpu).

Outside check mode nothing sees k_xfer_hostlink's iterations between the
first and the last — it has loops of its own, which the pair loops' probes
(tests/test_gpu_live_xfer.py) do not run.  Here one GPU rank and its endpoint
run one long unchecked call each, on threads of their own, and the test
thread watches the receiving end's rx while they run:

  the endpoint's rx  plain pinned host memory: poisoned with memset and read
                     by the test's own thread (message + 4 KiB guard);
  the GPU rank's rx  through mpx_fill / mpx_read on the context's utility
                     stream, beside the rank's kernel, as the pair cases do.

A counted probe proves every byte was rewritten after the poison, at >= 8
distinct times through the call.  The kernels are unmodified; tx is never
touched.  Each sizing call also gets the whole byte check.
"""
import ctypes as C

import numpy as np
import pytest

import mpx
import payload
import probe
from hostlink import SLACK, LinkMap
from test_gpu_live_xfer import POISON, RxSurface, probed

pytestmark = pytest.mark.gpu

PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
T = mpx.hostlink_ll_max()
BIG = (256 << 10) + 21
G, E = 0, 1


class HostRxSurface:
    """all of an endpoint's rx (pinned host memory), written and read by the
    calling thread; the first len(data) bytes are what the loop writes"""

    def __init__(self, rx, length: int, data: bytes):
        self.rx, self.length, self.poison_byte = rx, length, POISON
        self.expected = np.full(length, POISON, np.uint8)
        self.expected[:len(data)] = np.frombuffer(bytes(data), np.uint8)
        self.guards = np.ones(length, bool)
        self.guards[:len(data)] = False

    def poison(self):
        C.memset(self.rx, POISON, self.length)

    def snapshot(self):
        return np.frombuffer(self.rx, np.uint8, self.length).copy()


def host_case(request, capsys, mode, gpu_group, n, watch):
    """watch: "host" (the endpoint's rx) or "gpu" (the GPU rank's rx); that
    end receives the n bytes"""
    h = LinkMap(n, 2, [G], [E], [(G, E)])
    try:
        assert h.cap == n + SLACK
        if watch == "host":
            surface = HostRxSurface(h.host[E][1], h.cap, h.tx_bytes[G][:n])
        else:
            surface = RxSurface(h.c, h.gpu[G][1], h.cap, [(0, h.tx_bytes[E][:n])])
        other = E if watch == "gpu" else G

        def call(iters):
            h.reset_rx([other])
            out, errs = h.run([(G, E)], mode, gpu_group, n, iters, check=False, timeout_ms=5000)
            assert not errs, {k: str(e) for k, e in errs.items()}
            return out

        def verify(out, iters):
            # protocol, launches (1 on the GPU side, 0 on the host side), bytes, recv_done; tx of both ends;
            # and the whole rx of the end that is not watched (the watched one is the surface's)
            h.verify(out, [(G, E)], mode, gpu_group, n, iters, False, (mode, gpu_group, n, iters), rx_reset=False)
            grp = gpu_group if other == G else 1 - gpu_group
            payload.compare(h.rx(other), h.want_rx(other, G + E - other, mode, grp, n, iters), 0, "rx of the other end")

        what = f"host link mode {mode} GPU group {gpu_group} {n} B, watching the {watch} end"
        probed(request, capsys, what, surface, call, lambda out: max(t.wall_s for t in out.values()), verify)
    finally:
        h.close()


@pytest.mark.parametrize("n", [8, BIG])
def test_unidir_gpu_to_host_keeps_delivering(request, capsys, n):
    """8 B: LL granules into in.ll, unpacked by the endpoint's recv_ll every
    iteration; 256 KiB + 21: the kernel's bulk push into the endpoint's rx"""
    host_case(request, capsys, UNI, 1, n, "host")


@pytest.mark.parametrize("n", [8, BIG])
def test_unidir_host_to_gpu_keeps_delivering(request, capsys, n):
    """8 B: workgroup 0 polls out.ll across the link and unpacks; 256 KiB + 21:
    every workgroup pulls its chunk of the endpoint's tx"""
    host_case(request, capsys, UNI, 0, n, "gpu")


def test_pingpong_keeps_delivering(request, capsys):
    """4161 B ping-pong, probing the endpoint's rx"""
    host_case(request, capsys, PP, 1, 4161, "host")
