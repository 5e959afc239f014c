"""k_copy's resident window on the GPU (run with -m gpu).

k_copy_win picks the load's cache policy per workgroup: 4 KiB block b of
src is loaded with the default policy (a buffer load) when
(b / unit) % period < window, and nontemporal (a pointer load) otherwise;
stores and the tail bytes are the plain kernel's.  The policy must never show
in the bytes: every forced window, at sizes with a partial last block, tail
bytes and less than one period, from interior pointers, copies src exactly and
writes nothing past dst + n.  MPX_COPY=launch sends the small sizes to a launch per copy.
The rule itself (copy_window_rule) is held by tests/test_copy_window.py; here
one case runs it with no knob at the size where it turns on, below it, and at
the headline's 1 GiB.
"""
import pytest

import mpx
import oracle_py as O
import payload
from payload import assert_region, sub

pytestmark = pytest.mark.gpu

TOTAL = (1 << 20) + (16 << 10)
KEY = mpx.pattern_key(mpx.PATTERN_SEED, 6, 2, 9)
SIZES = [4080, 4096, 4112, 8192 + 13, 12288, 65536 + 4096 + 5, (1 << 20) + 13]
WINDOWS = ["8192:0", "8192:8192", "8192:4096", "65536:12288", "65536:12288:8192"]
OFFSETS = [(16, 4080), (4080, 16)]       # (src, dst): 16-byte aligned, not block aligned
RULE_ON = 512 << 20                      # kCopyWindowMin (mpx_internal.h)


@pytest.fixture(scope="module")
def ctx():
    c = mpx.Context(2, "kernel")
    yield c
    c.close()


@pytest.fixture(scope="module")
def bufs(ctx):
    """src: seeded once over the whole allocation, never written again"""
    src, dst = ctx.alloc(0, TOTAL), ctx.alloc(0, TOTAL)
    ctx.fill(src, TOTAL, mpx.FILL_SPLITMIX, KEY)
    host = O.fill(TOTAL, mpx.FILL_SPLITMIX, KEY)
    payload.compare(ctx.read(src, TOTAL), host, 0, "seeded src")
    yield src, dst, host
    ctx.free(src)
    ctx.free(dst)


@pytest.mark.parametrize("window", WINDOWS)
def test_forced_windows_copy_every_byte_and_nothing_else(ctx, bufs, monkeypatch, window):
    """all nontemporal, all kept, alternate blocks, 3 of 16 blocks, 3 of 16
    two-block units: dst[0:n) == src[0:n), 64 poisoned bytes on either side
    untouched, one copy and three"""
    src, dst, host = bufs
    monkeypatch.setenv("MPX_COPY", "launch")
    monkeypatch.setenv("MPX_COPY_WINDOW", window)
    for soff, doff in OFFSETS:
        for n in SIZES:
            for iters in (1, 3):
                ctx.fill(dst, TOTAL, mpx.FILL_BYTE, payload.GUARD_BYTE)
                t = ctx.copy(0, sub(dst, doff), sub(src, soff), n, iters)
                assert mpx.PROTOCOLS.get(t.protocol) == "copy" and t.launches == iters and t.bytes == n * iters
                assert t.nwg == (n // 16 + 255) // 256
                assert_region(ctx, dst, doff, host[soff:soff + n],
                              what=f"window {window}: src+{soff} -> dst+{doff}, {n} B x {iters}")


def test_window_off_and_sizes_below_one_unit(ctx, bufs, monkeypatch):
    """"0" is the kernel without the choice; a forced window also holds for
    n < 16 (tail bytes only) and n = 0"""
    src, dst, host = bufs
    monkeypatch.setenv("MPX_COPY", "launch")
    for window in ("0", "8192:8192"):
        monkeypatch.setenv("MPX_COPY_WINDOW", window)
        for n in (0, 1, 15, 16, 17, 4096 + 5):
            ctx.fill(dst, TOTAL, mpx.FILL_BYTE, payload.GUARD_BYTE)
            ctx.copy(0, sub(dst, 4080), sub(src, 16), n, 2)
            assert_region(ctx, dst, 4080, host[16:16 + n], what=f"window {window}: {n} B")


@pytest.mark.parametrize("bad", ["1", "4096", "8192", "8192:", "8192:4097", "8191:4096", "8192:12288", "12288:4096",
                                 "8192:4096:12288", "8192:4096:0", "8192:4096:4096:4096", "x", "8192;4096"])
def test_malformed_windows_are_refused(ctx, bufs, monkeypatch, bad):
    """MPX_ERR_INVALID before any launch, whatever form the size would take"""
    src, dst, _ = bufs
    monkeypatch.setenv("MPX_COPY_WINDOW", bad)
    ctx.fill(dst, 8192, mpx.FILL_BYTE, payload.GUARD_BYTE)
    for how in ("launch", None):
        if how:
            monkeypatch.setenv("MPX_COPY", how)
        else:
            monkeypatch.delenv("MPX_COPY", raising=False)
        with pytest.raises(mpx.MpxError) as e:
            ctx.copy(0, dst, src, 4096, 2)
        assert e.value.status == mpx.ERR_INVALID, bad
    assert ctx.read(dst, 8192) == bytes([payload.GUARD_BYTE]) * 8192


def test_default_rule_at_its_threshold_and_the_headline_size(ctx, monkeypatch):
    """no knob: the rule's own window where it turns on (512 MiB), the plain
    kernel one byte below, and 1 GiB.  dst's checksum equals src's, the first
    and last 8 KiB read back equal, and the 64 bytes after dst + n keep their
    poison."""
    monkeypatch.delenv("MPX_COPY", raising=False)
    monkeypatch.delenv("MPX_COPY_WINDOW", raising=False)
    big = 1 << 30
    src, dst = ctx.alloc(0, big), ctx.alloc(0, big + 4096)
    try:
        ctx.fill(src, big, mpx.FILL_SPLITMIX, KEY)
        head = O.fill(8192, mpx.FILL_SPLITMIX, KEY)
        assert ctx.read(src, 8192) == head
        for n in (RULE_ON, RULE_ON - 1, big):
            ctx.fill(dst, big + 4096, mpx.FILL_BYTE, payload.GUARD_BYTE)
            t = ctx.copy(0, dst, src, n, 2)
            assert mpx.PROTOCOLS.get(t.protocol) == "copy" and t.launches == 2
            assert ctx.checksum(dst, n) == ctx.checksum(src, n), n
            assert ctx.read(dst, 8192) == head, n
            last = n - 8192
            assert ctx.read(dst, 8192 + 64, offset=last) == \
                ctx.read(src, 8192, offset=last) + bytes([payload.GUARD_BYTE]) * 64, n
    finally:
        ctx.free(src)
        ctx.free(dst)
