"""Mid-call probes of mpx_copy's loops (tests/probe.py; run with -m gpu).

test_gpu_engine.py and test_gpu_bytes.py compare dst with the pattern after
the call, which shows the last of the call's `iters` copies and nothing of the
ones before it.  Here dst — and in half of the cases src too — lies in
host-mapped memory, which mpx_copy takes like any other 16-byte-aligned
device-visible pointer, and the CPU reads and writes those bytes while the
kernel runs: it poisons dst with its guards and waits for the payload to come
back (store probe), or gives src its other pattern and waits for dst to follow
(load probe: each of the `iters` copies loads src anew, include/mpx.h).  The
kernels are the ones the device-memory tests run: same instantiations, same
grid rule, chosen by n and MPX_COPY.

The launch-per-copy form comes first: every copy is a kernel of its own
there, so it is the reference for the harness.  A one-launch case that counts
fewer probes than the mark where the launch form counts them says something
about the loop, not about the observer.

Two things the observer needs on an MI355X, both measured:

* The memory is hipHostMalloc(Portable | Mapped | Uncached), the GPU's
  MTYPE_UC pool.  In plain coherent host memory (Mapped | Coherent) the copy
  kernels' nontemporal stores, which carry no system scope, stay in the GPU's
  L2 until the kernel ends: every one-launch form showed its first payload
  361-398 ms into a 362-398 ms call, the launch form after 0.3 ms.
* A load probe needs the loop's next loads of src to miss the CU's vector
  L1, which nothing invalidates inside a kernel.  Workgroups that re-read 16
  KiB or more per copy followed a rewritten src by themselves (thousands of
  load probes in 0.4 s); workgroups of 256 or 512 lanes with one unit per lane
  and k_copy_pipe with one unit per lane (4-8 KiB per workgroup and copy)
  counted 0-3.  So while a load probe waits, the observer runs a 16 MiB copy
  of its own on a second context's stream, which sweeps every CU's L1: then
  all of them count thousands.  A loop whose loads sit above its step loop
  does not follow whatever is evicted (hand control (a), README).
"""
import ctypes as C

import numpy as np
import pytest

import mpx
import oracle_py as O
import payload
import probe

pytestmark = pytest.mark.gpu

G = payload.GUARD
POISON = payload.GUARD_BYTE
HOST_CAP = (1 << 20) + 4096
EVICT = 16 << 20                  # the observer's own copy: 4096 workgroups, 64 KiB through every CU
HIP_HOST_MALLOC_PORTABLE, HIP_HOST_MALLOC_MAPPED, HIP_HOST_MALLOC_UNCACHED = 0x1, 0x2, 0x10000000
DEADLINES = dict(start_deadline_s=2.0, probe_deadline_s=2.0, join_deadline_s=30.0)
KEYS = [mpx.pattern_key(mpx.PATTERN_SEED, 11, 12, k) for k in (1, 2)]


class HostBuf:
    """uncached host-mapped memory: .arr the CPU's view, .ptr the GPU's pointer"""

    def __init__(self, size: int):
        h = payload.hip()
        h.hipHostMalloc.restype = h.hipHostGetDevicePointer.restype = h.hipHostFree.restype = C.c_int
        h.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        h.hipHostGetDevicePointer.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint]
        h.hipHostFree.argtypes = [C.c_void_p]
        self.h, self.size = h, size
        hp, dp = C.c_void_p(), C.c_void_p()
        rc = h.hipHostMalloc(C.byref(hp), size, HIP_HOST_MALLOC_PORTABLE | HIP_HOST_MALLOC_MAPPED
                             | HIP_HOST_MALLOC_UNCACHED)
        assert rc == 0 and hp.value, f"hipHostMalloc({size}): hip error {rc}"
        self.host = hp.value
        rc = h.hipHostGetDevicePointer(C.byref(dp), hp, 0)
        assert rc == 0 and dp.value and dp.value % 4096 == 0, (rc, dp.value)
        self.ptr = dp.value
        self.arr = np.ctypeslib.as_array((C.c_ubyte * size).from_address(self.host))
        self.arr[:] = 0

    def free(self):
        self.arr = None
        assert self.h.hipHostFree(C.c_void_p(self.host)) == 0


@pytest.fixture(scope="module")
def box():
    """one context, host memory for dst and src, device memory for src; a
    second context whose utility stream is free while mpx_copy holds the first
    one's: HostBuf.evict, the observer's 16 MiB copy (module docstring)"""
    c, c2 = mpx.Context(1, "kernel"), mpx.Context(1, "kernel")
    hd, hs = HostBuf(HOST_CAP), HostBuf(HOST_CAP)
    ds, ev = c.alloc(0, HOST_CAP), [c2.alloc(0, EVICT), c2.alloc(0, EVICT)]
    hs.evict = lambda: c2.copy(0, ev[0], ev[1], EVICT, 1)
    yield c, hd, hs, ds
    c2.free(ev[0])
    c2.free(ev[1])
    c2.close()
    c.free(ds)
    c.close()
    hd.free()
    hs.free()


def pattern(k: int, n: int) -> np.ndarray:
    return np.frombuffer(O.fill(n, mpx.FILL_SPLITMIX, KEYS[k]), np.uint8)


class CopySurface:
    """dst = hd[64 : 64 + n) with 64 guard bytes either side, all of it host
    memory.  src: host memory (hs given; rewrite() for load probes) or
    device memory filled with pattern 0."""

    def __init__(self, hd: HostBuf, n: int, hs=None):
        src_arr = hs.arr if hs is not None else None
        self.evict = hs.evict if hs is not None else None
        self.n, self.poison_byte = n, POISON
        self.mem = hd.arr[:G + n + G]
        self.dst = mpx.Buffer(hd.ptr + G, 0, n)
        self.pat = [pattern(0, n), pattern(1, n)]
        assert ((self.pat[0] != self.pat[1]).mean() > 0.99) if n >= 4096 else (self.pat[0] != self.pat[1]).any()
        self.k, self.rewritten = 0, False
        self.src_arr = src_arr
        if src_arr is not None:
            src_arr[:n] = self.pat[0]
        self.expected = np.full(G + n + G, POISON, np.uint8)
        self.expected[G:G + n] = self.pat[0]
        self.guards = np.ones(G + n + G, bool)
        self.guards[G:G + n] = False

    def poison(self):
        self.mem[:] = POISON
        self.rewritten = False

    def snapshot(self):
        if self.rewritten:          # a load probe is waiting: sweep the CUs' L1
            self.evict()
        return self.mem.copy()

    def rewrite(self):
        self.k ^= 1
        self.src_arr[:self.n] = self.pat[self.k]
        self.expected[G:G + self.n] = self.pat[self.k]
        self.rewritten = True

    def locate(self, off: int) -> str:
        return f"dst {off - G:+d} of {self.n}"


K = 1 << 10
N_MID = 128 * K + 33
# (MPX_COPY, n, mpx_timing.protocol, what it is there for)
CASES = [
    ("launch", 4096 + 5, "copy", "a kernel per copy: the harness's reference"),
    ("steps", 17, "copy_steps", "one unit and a tail, one workgroup"),
    ("steps", 16 * K + 17, "copy_steps", "first multi-workgroup class, one XCD"),
    ("steps", N_MID, "copy_steps", "512 -> 1024 lanes, one XCD"),
    ("steps", 512 * K + 3, "copy_steps", "every XCD, 1024 lanes"),
    ("steps:16:0:0:1:1024", N_MID, "copy_steps", "one counter (xcd 0), grid capped at 16"),
    ("steps:64:1:0:1:256", N_MID, "copy_steps", "per-XCD counters (xcd 1), 33 workgroups"),
    ("steps:64:0:1:1:512", N_MID, "copy_steps", "drain 1"),
    ("steps:64:0:0:1:256", N_MID, "copy_steps", "256 lanes"),
    ("steps:64:0:0:1:512", N_MID, "copy_steps", "512 lanes"),
    ("steps:64:0:0:1:1024", N_MID, "copy_steps", "1024 lanes"),
    ("steps:32:0:0:1:1024:1", N_MID, "copy_steps", "one_xcd"),
    ("steps:64:0:0:8:256", (1 << 20) + 3, "copy_steps", "batched: four units per lane"),
    ("pipe:1:0", 17, "copy_pipe", "grid of one"),
] + [(f"pipe:{upl}:{hier}", 256 * K + 16 + 5, "copy_pipe", "units per lane x barrier form")
     for upl in (1, 4, 16) for hier in (0, 1)]


@pytest.mark.parametrize("src_in", ["device", "host"])
@pytest.mark.parametrize("form,n,proto", [c[:3] for c in CASES], ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_copy_loop_keeps_moving_its_bytes(box, monkeypatch, request, capsys, form, n, proto, src_in):
    """A short unprobed call (2000 copies: byte check, and the size of the
    probed call, about 0.4 s), then the probed call: at least 8 counted store
    probes — and with src in host memory as many load probes, the two
    alternating — and at most one inconclusive probe, the last; protocol,
    launches and bytes as reported (a fall-back to a launch per copy cannot
    pass as the one-launch form)."""
    ctx, hd, hs, ds = box
    monkeypatch.setenv("MPX_COPY", form)
    host_src = src_in == "host"
    s = CopySurface(hd, n, hs if host_src else None)
    if host_src:
        src = mpx.Buffer(hs.ptr, 0, n)
    else:
        src = ds
        ctx.fill(ds, n, mpx.FILL_SPLITMIX, KEYS[0])

    def verify(t, iters):
        assert (mpx.PROTOCOLS[t.protocol], t.launches, t.bytes) == \
            (proto, iters if proto == "copy" else 1, n * iters), (form, n, t.as_dict())

    s.poison()
    t = ctx.copy(0, s.dst, src, n, probe.SIZING_ITERS)
    verify(t, probe.SIZING_ITERS)
    payload.compare(s.snapshot().tobytes(), s.expected.tobytes(), -G, f"{form} {n} B: dst after the sizing call")
    iters = probe.size_iters(t.wall_s)

    kinds = ("store", "load") if host_src else ("store",)
    rep = probe.run_probed(lambda: ctx.copy(0, s.dst, src, n, iters), s, load=host_src, poll_sleep_s=None,
                           iters=iters, **DEADLINES)
    probe.say(request, capsys, f"{form} {n} B src {src_in}: {rep}; sizing call {t.wall_s * 1e3:.2f} ms, probed call "
                                f"{rep.result.wall_s * 1e3:.1f} ms")
    verify(rep.result, iters)
    probe.require(rep, kinds)
