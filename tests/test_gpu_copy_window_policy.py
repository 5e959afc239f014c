"""k_copy_win's cache policies never show in the bytes (run with -m gpu).

The kernel picks a cache policy per workgroup for its loads and carries one on
its stores (tests/test_copy_window_policy.py reads them in the emitted code).
Whatever they are, a copy is exact at every block and stripe edge and complete
when its launch ends: through mpx_copy with MPX_COPY_WINDOW forced, dst equals
the seeded source byte for byte, the guard bytes around it keep their poison,
the oracle's checksum of the host pattern is dst's, and a source rewritten
between two copies is never served from a kept line.

Windows are written here as (period, window) in units and the unit in bytes;
MPX_COPY_WINDOW takes period and window x 4096.
"""
import pytest

import mpx
import oracle_py as O
import payload
from payload import assert_region, sub

pytestmark = pytest.mark.gpu

BLOCK = 4096
TOTAL = (1 << 20) + (16 << 10)
KEY = mpx.pattern_key(mpx.PATTERN_SEED, 6, 2, 9)       # tests/test_gpu_copy_window.py's pattern
KEY2 = mpx.pattern_key(mpx.PATTERN_SEED, 6, 2, 10)
SOFF, DOFF = 16, 4080                                  # 16-byte aligned, not block aligned
# one unit; one unit short of a block; a block; a block and tail bytes; a last
# block of one unit at block index 255 (kept by 32:32 alone) and at 256 (kept
# by every window below but "0"); many blocks, a partial one and tail bytes
SIZES = [16, 4080, 4096, 4096 + 13, 255 * BLOCK + 16, 256 * BLOCK + 16, (1 << 20) + 4096 + 7]
WINDOWS = {"8:3:4096": (8, 3, 4096), "2:1:4096": (2, 1, 4096), "32:32:4096": (32, 32, 4096), "0": None}


def knob(window):
    if window is None:
        return "0"
    period, win, unit = window
    return f"{period * BLOCK}:{win * BLOCK}:{unit}"


def kept(window, block):
    if window is None:
        return False
    period, win, unit = window
    return (block // (unit // BLOCK)) % period < win


def test_the_cases_are_the_edges_they_are_named_for():
    """the last block of 255 x 4096 + 16 is partial, kept by 32:32 and streamed
    by the striped windows; that of 256 x 4096 + 16 is kept by all three"""
    assert [kept(WINDOWS[w], 255) for w in ("8:3:4096", "2:1:4096", "32:32:4096", "0")] == [False, False, True, False]
    assert [kept(WINDOWS[w], 256) for w in ("8:3:4096", "2:1:4096", "32:32:4096", "0")] == [True, True, True, False]
    assert max(SIZES) + max(SOFF, DOFF) + payload.GUARD <= TOTAL


@pytest.fixture(scope="module")
def ctx():
    c = mpx.Context(2, "kernel")
    yield c
    c.close()


@pytest.fixture(scope="module")
def bufs(ctx):
    """src seeded once; the host pattern and its checksums per size computed once"""
    src, dst = ctx.alloc(0, TOTAL), ctx.alloc(0, TOTAL)
    ctx.fill(src, TOTAL, mpx.FILL_SPLITMIX, KEY)
    host = O.fill(TOTAL, mpx.FILL_SPLITMIX, KEY)
    payload.compare(ctx.read(src, TOTAL), host, 0, "seeded src")
    sums = {n: O.checksum(host[SOFF:SOFF + n]) for n in SIZES}
    yield src, dst, host, sums
    ctx.free(src)
    ctx.free(dst)


@pytest.mark.parametrize("window", list(WINDOWS))
def test_every_policy_copies_every_byte_at_block_and_stripe_edges(ctx, bufs, monkeypatch, window):
    src, dst, host, sums = bufs
    monkeypatch.setenv("MPX_COPY", "launch")
    monkeypatch.setenv("MPX_COPY_WINDOW", knob(WINDOWS[window]))
    for n in SIZES:
        for iters in (1, 3):
            ctx.fill(dst, TOTAL, mpx.FILL_BYTE, payload.GUARD_BYTE)
            t = ctx.copy(0, sub(dst, DOFF), sub(src, SOFF), n, iters)
            assert mpx.PROTOCOLS.get(t.protocol) == "copy" and t.launches == iters and t.bytes == n * iters
            what = f"window {window}: {n} B x {iters}"
            assert_region(ctx, dst, DOFF, host[SOFF:SOFF + n], what=what)
            assert ctx.checksum(sub(dst, DOFF), n) == sums[n], what


@pytest.mark.parametrize("window", ["8:3:4096", "32:32:4096"])
def test_a_rewritten_source_is_never_served_from_a_kept_line(ctx, monkeypatch, window):
    """copy (twice: the second copy reads what the first kept), overwrite src
    with a second seed, copy again: dst is the second pattern"""
    n = (1 << 20) + 4096 + 7
    monkeypatch.setenv("MPX_COPY", "launch")
    monkeypatch.setenv("MPX_COPY_WINDOW", knob(WINDOWS[window]))
    src, dst = ctx.alloc(0, TOTAL), ctx.alloc(0, TOTAL)
    try:
        ctx.fill(dst, TOTAL, mpx.FILL_BYTE, payload.GUARD_BYTE)
        for key in (KEY, KEY2):
            ctx.fill(src, TOTAL, mpx.FILL_SPLITMIX, key)
            ctx.copy(0, sub(dst, DOFF), sub(src, SOFF), n, 2)
            want = O.fill(TOTAL, mpx.FILL_SPLITMIX, key)[SOFF:SOFF + n]
            assert_region(ctx, dst, DOFF, want, what=f"window {window}, key {key:#x}")
            assert ctx.checksum(sub(dst, DOFF), n) == O.checksum(want)
    finally:
        ctx.free(src)
        ctx.free(dst)
