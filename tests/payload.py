"""Byte-exact payload helpers for the -m gpu tests (tests/test_gpu_bytes.py).

TEST INFRASTRUCTURE: plain functions, no fixtures.  Everything a test expects
comes from the host (oracle_py.fill / oracle_py.checksum of host bytes); this
module only restates the chunk arithmetic, writes arbitrary host bytes into a
device buffer, and compares a device region with its guards byte for byte.
"""
from __future__ import annotations

import ctypes as C

import mpx

MIN_PUSH_CHUNK = 1024      # kMinPushChunk (mpx_internal.h): bytes per workgroup, at least
GUARD = 64
GUARD_BYTE = 0xEE


def chunk_shape(nwg: int, n: int):
    """(width, chunk, empty workgroups, last non-empty workgroup, its bytes) of
    a bulk message of n bytes at the explicit width nwg: run_kernel's
    narrowing (at least kMinPushChunk bytes per workgroup, at least one
    workgroup) and Loop::chunk_of (ceil(n / width) rounded up to 16 B;
    workgroup w owns [w * chunk, min((w + 1) * chunk, n))).  n = 0: one
    workgroup, empty; last = -1."""
    width = max(1, min(nwg, -(-n // MIN_PUSH_CHUNK)))
    chunk = (-(-n // width) + 15) & ~15
    if n == 0:
        return width, chunk, width, -1, 0
    empty = sum(1 for w in range(width) if w * chunk >= n)
    last = (n - 1) // chunk
    return width, chunk, empty, last, n - last * chunk


# (nwg, n) -> the chunk properties each case is there for: (width, chunk,
# empty workgroups, last non-empty workgroup, its bytes).  Written out, not
# computed: tests/test_payload_cases.py holds chunk_shape against them, so a
# change of kMinPushChunk or of the rounding cannot quietly turn them into
# ordinary cases.  (256, 456131) is the reference's own message size
# (scripts/run-hbv3.sh) at the widest width bench.py's tuner tries.
EDGE_CASES = {
    (256, 456131): (256, 1792, 1, 254, 963),        # tail 3
    (70, 71681): (70, 1040, 1, 68, 961),
    (256, 262145): (256, 1040, 3, 252, 65),
    (200, 204801): (200, 1040, 3, 196, 961),
    (65, 66561): (65, 1040, 0, 64, 1),              # no 16-B unit, only a tail
    (256, (1 << 20) + 1): (256, 4112, 0, 255, 17),  # one unit + 1
}

NB_WINDOW = 256           # kNbWindow (mpx_internal.h)


def ring_bytes_for(length: int, cap: int = 64 << 20) -> int:
    """bytes of the check-mode receive ring of a rank attached with `length`
    bytes (ring_bytes_for, mpx_runtime.hip): whole slots of the attached
    length, at most 255, within `cap` = MPX_CHECK_RING_BYTES"""
    if length == 0:
        return 0
    return min((NB_WINDOW - 1) * length, cap) // length * length


def ring_slots(ring_bytes: int, n: int) -> int:
    """receive slots of a link for messages of n bytes (ring_slots,
    mpx_internal.h): rx itself and every whole message the ring holds"""
    return NB_WINDOW if n <= 0 else min(NB_WINDOW, 1 + ring_bytes // n)


_hip = None


def hip():
    """the HIP runtime libmpx runs on (tools/link_counter_control.py binds it
    the same way)"""
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so.7")
        h.hipMemcpy.restype = C.c_int
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip = h
    return _hip


HIP_MEMCPY_HOST_TO_DEVICE = 1


def write(ctx, buf, data: bytes, offset: int = 0) -> None:
    """buf[offset : offset + len(data)) = data, synchronously (hipMemcpy).
    Only between calls: no transfer kernel of the context may be in flight."""
    data = bytes(data)
    assert 0 <= offset and offset + len(data) <= buf.size, (offset, len(data), buf.size)
    if not data:
        return
    src = C.create_string_buffer(data, len(data))
    rc = hip().hipMemcpy(C.c_void_p(buf.ptr + offset), src, len(data), HIP_MEMCPY_HOST_TO_DEVICE)
    if rc != 0:
        raise RuntimeError(f"hipMemcpy of {len(data)} B to {buf.ptr + offset:#x}: hip error {rc}")


def sub(buf, off: int):
    """the buffer from byte `off` of buf on (an interior pointer)"""
    assert 0 <= off <= buf.size, (off, buf.size)
    return mpx.Buffer(buf.ptr + off, buf.dev, buf.size - off)


def _hex(b: bytes) -> str:
    return b.hex(" ") if b else "(none)"


def compare(got: bytes, want: bytes, base: int = 0, what: str = "") -> None:
    """got == want, or an AssertionError that says where: the first differing
    offset (counted from `base`, the buffer offset of got[0]), how many bytes
    differ, and 16 bytes of each around the first difference."""
    if got == want:
        return
    if len(got) != len(want):
        raise AssertionError(f"{what}: read {len(got)} bytes, expected {len(want)}")
    diff = [i for i in range(len(want)) if got[i] != want[i]]
    i = diff[0]
    lo = max(0, i - 8)
    raise AssertionError(
        f"{what}: {len(diff)} of {len(want)} bytes differ, first at offset {base + i} "
        f"(last at {base + diff[-1]}); bytes [{base + lo}, {base + lo + 16}): "
        f"got {_hex(got[lo:lo + 16])} want {_hex(want[lo:lo + 16])}")


def region(off: int, expect: bytes, size: int, guard: int = GUARD, fill: int = GUARD_BYTE):
    """(start, expected bytes) of the guarded region around buf[off : off +
    len(expect)): `guard` bytes of `fill` on either side.  The front guard is
    cut at the start of the buffer; the rear one must fit."""
    front = min(guard, off)
    assert off >= 0 and off + len(expect) + guard <= size, (off, len(expect), guard, size)
    return off - front, bytes([fill]) * front + bytes(expect) + bytes([fill]) * guard


def assert_region(ctx, buf, off: int, expect: bytes, guard: int = GUARD, fill: int = GUARD_BYTE, what: str = ""):
    """buf[off : off + len(expect)) == expect and the `guard` bytes before and
    after still hold `fill` (read back with ctx.read, compared on the host)"""
    start, want = region(off, expect, buf.size, guard, fill)
    compare(ctx.read(buf, len(want), offset=start), want, start, what or f"buffer {buf.ptr:#x}")
