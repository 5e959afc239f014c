"""Byte-exact payload checks at chunk, LL and pointer edges (-m gpu, MI355X).

The pair tests elsewhere decide "rx is right" with one device checksum against
another, mostly under the reference's constant fill ('a' / 'b'), where the
checksum cannot see a misplaced, permuted or duplicated word
(tests/test_payload_cases.py pins that down).  Here every expectation is host
bytes: oracle_py.fill for seeded buffers, or the very bytes payload.write put
into tx; rx is read back and compared byte for byte with 64 guard bytes
around it (payload.assert_region), the receive digest is recomputed on the
host (oracle_py.checksum), and tx is read back unchanged.  Pairs are loopback
ranks on GPU 0 (tests/pairs.py), whose in-kernel check is told the host's
checksums too (HostPairs.expect).

  B  bulk messages whose last workgroups hold an empty or tail-only chunk
  C  ragged LL messages, adversarial contents, negative controls
  D  the copy kernels at interior (16-byte aligned) pointers
  E  mpx_fill / mpx_checksum: the alignment contract, interior pointers
"""
import numpy as np
import pytest

import mpx
import oracle_py as O
import payload
from hostpairs import HostPairs, run_checked
from payload import assert_region, chunk_shape, sub

pytestmark = pytest.mark.gpu

PINGPONG, NONBLOCKING, UNIDIR = mpx.MODE_PINGPONG, mpx.MODE_NONBLOCKING, mpx.MODE_UNIDIR
PROTO_LL, PROTO_BULK, PROTO_PULL = 0, 1, 7
GUARD = payload.GUARD


# --------------------------------------------------------------------------
# B. empty and tail-only chunks
# --------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["push", "push_stream", "pull"])
@pytest.mark.parametrize("mode", [PINGPONG, NONBLOCKING, UNIDIR])
def test_empty_and_tail_only_chunks(mode, how):
    """Explicit widths at which chunk_of's rounding leaves the last workgroups
    nothing (lo >= n) or only a tail: they move no byte, and must still
    publish their flag (push), return their credit and landed count (pull),
    count their chunk in (non-blocking check) and add 0 to the checksum."""
    kw = {"push": {}, "push_stream": {"stream": True}, "pull": {"pull": True}}[how]
    P = HostPairs(max(n for _, n in payload.EDGE_CASES) + GUARD)
    try:
        for (nwg, n), claimed in payload.EDGE_CASES.items():
            assert chunk_shape(nwg, n) == claimed
            out = run_checked(P, mode, n, 3, (how, mode, nwg, n), nwg=nwg, **kw)
            for r in (0, 1):
                assert out[r].nwg == claimed[0], (nwg, n, r, out[r].nwg)
                assert out[r].protocol == (PROTO_PULL if how == "pull" else PROTO_BULK), (nwg, n, r)
    finally:
        P.close()


# --------------------------------------------------------------------------
# C. ragged LL messages
# --------------------------------------------------------------------------
LL_DEFAULT_MAX = 2048      # ll_max_bytes(same_device)
LL_SIZES_DEFAULT = list(range(0, 18)) + list(range(2033, 2050))
# 255, 256, 257 units; 512, 513; 768, 769; 1023, 1024 — last units of one and
# of two granules, last granules of 1-4 bytes
LL_SIZES_8K = ([2040, 2041, 2047, 2048, 2049, 2055, 2056, 2057] + list(range(4089, 4098)) + [6143, 6144, 6145]
               + list(range(8184, 8193)))


@pytest.mark.parametrize("mode", [PINGPONG, UNIDIR])
def test_ll_ragged_sizes_default_threshold(mode):
    """Every n % 8 at the start of the landing zone and at the loopback LL
    threshold: the unpack's byte stores, preload_ll's byte loop, the
    one-granule last unit; LL up to 2048 B, bulk at 2049."""
    P = HostPairs(2049 + GUARD)
    try:
        for n in LL_SIZES_DEFAULT:
            out = run_checked(P, mode, n, 5, ("ll", mode, n))
            for r in (0, 1):
                assert out[r].protocol == (PROTO_LL if n <= LL_DEFAULT_MAX else PROTO_BULK), (n, r, out[r].protocol)
    finally:
        P.close()


@pytest.mark.parametrize("pull", [False, True])
@pytest.mark.parametrize("mode", [PINGPONG, UNIDIR])
def test_ll_ragged_sizes_whole_landing_zone(monkeypatch, mode, pull):
    """The cross-GPU threshold (8 KiB) on a loopback link: the lane boundaries
    of the landing zone (one to four units per lane), ragged on both sides
    of each; pulled calls keep LL messages pushes."""
    monkeypatch.setenv("MPX_LL_MAX", "8192")
    P = HostPairs(8192 + GUARD)
    try:
        for n in LL_SIZES_8K:
            out = run_checked(P, mode, n, 5, ("ll8k", mode, pull, n), pull=pull)
            for r in (0, 1):
                assert out[r].protocol == PROTO_LL, (n, r, out[r].protocol)
    finally:
        P.close()


ADV_ITERS = 5
ADV_LL, ADV_BULK, ADV_BULK_NWG = 2045, 71681, 70


def _adversarial(kind: str, n: int) -> bytes:
    if kind == "zeros":        # a zeroed mailbox, a never-written rx
        return bytes(n)
    if kind == "ones":
        return b"\xff" * n
    if kind == "tags":         # ll_tag of a fresh link's first sequence numbers, as payload words
        words = b"".join((0x80000001 + k).to_bytes(4, "little") for k in range(16))
        return (words * (n // len(words) + 1))[:n]
    if kind == "poison":       # check mode's poison bytes of the iterations run
        cyc = bytes(0x5a ^ i for i in range(ADV_ITERS))
        return (cyc * (n // len(cyc) + 1))[:n]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["zeros", "ones", "tags", "poison"])
@pytest.mark.parametrize("mode", [PINGPONG, UNIDIR])
def test_adversarial_content(mode, kind):
    """Payloads that look like the protocol's own words: a payload word is
    never taken for a tag, a stale unit never for a fresh one, and a payload
    equal to the poison or to untouched memory is still delivered (the 0xEE
    prefill shows it)."""
    P = HostPairs(ADV_BULK + GUARD)
    try:
        data = _adversarial(kind, ADV_BULK)
        P.set_tx(data)
        for r in (0, 1):
            assert P.host[r][:ADV_BULK] == data
        out = run_checked(P, mode, ADV_LL, ADV_ITERS, (kind, mode, "ll"))
        assert all(out[r].protocol == PROTO_LL for r in (0, 1))
        out = run_checked(P, mode, ADV_BULK, ADV_ITERS, (kind, mode, "bulk"), nwg=ADV_BULK_NWG)
        assert all(out[r].protocol == PROTO_BULK and out[r].nwg == ADV_BULK_NWG for r in (0, 1))
    finally:
        P.close()


@pytest.mark.parametrize("n,nwg,left", [(ADV_BULK, ADV_BULK_NWG, 0xEE), (ADV_LL, 0, 0xFF)])
@pytest.mark.parametrize("mode", [PINGPONG, UNIDIR])
def test_lost_payload_fails_the_byte_comparison(monkeypatch, mode, n, nwg, left):
    """Negative control on the device path (MPX_TEST=skip_push=1: the only
    push of an unchecked one-iteration call moves no payload, every flag and
    tag still goes): the call succeeds, rx keeps the prefill (bulk) or holds
    the knob's fixed wrong words (LL), and the byte comparison raises."""
    monkeypatch.setenv("MPX_TEST", "skip_push=1")
    P = HostPairs(n + GUARD)
    try:
        for r in (0, 1):
            P.c.fill(P.bufs[r][1], n + GUARD, mpx.FILL_BYTE, payload.GUARD_BYTE)
        out, errs = P.run(mode, n, 1, check=False, nwg=nwg)
        assert not errs, errs
        for r in ((0, 1) if mode == PINGPONG else (1,)):      # the ranks that receive the B-byte payload
            rx = P.bufs[r][1]
            assert_region(P.c, rx, 0, bytes([left]) * n, what=f"rx of rank {r} after a lost payload")
            with pytest.raises(AssertionError, match="bytes differ, first at offset"):
                assert_region(P.c, rx, 0, P.host[P.peer(r)][:n])
    finally:
        P.close()


# --------------------------------------------------------------------------
# D. copy kernels at interior pointers
# --------------------------------------------------------------------------
COPY_TOTAL = 512 << 10
COPY_KEY = mpx.pattern_key(mpx.PATTERN_SEED, 4, 4, 4)
OFFSETS = [(0, 64), (16, 80), (4080, 4080), (16, 4096 + 48)]


@pytest.fixture(scope="module")
def ctx():
    c = mpx.Context(2, "kernel")
    yield c
    c.close()


@pytest.fixture(scope="module")
def copy_bufs(ctx):
    """src: seeded over the whole allocation, never written again; dst:
    refilled with 0xEE before every copy"""
    src, dst = ctx.alloc(0, COPY_TOTAL), ctx.alloc(0, COPY_TOTAL)
    ctx.fill(src, COPY_TOTAL, mpx.FILL_SPLITMIX, COPY_KEY)
    host = O.fill(COPY_TOTAL, mpx.FILL_SPLITMIX, COPY_KEY)
    payload.compare(ctx.read(src, COPY_TOTAL), host, 0, "seeded src")
    yield src, dst, host
    ctx.free(src)
    ctx.free(dst)


def _copies(ctx, copy_bufs, sizes, iters_list, protocol):
    src, dst, host = copy_bufs
    for soff, doff in OFFSETS:
        for n in sizes:
            assert soff + n <= COPY_TOTAL and doff + n + GUARD <= COPY_TOTAL and doff >= GUARD
            for iters in iters_list:
                ctx.fill(dst, COPY_TOTAL, mpx.FILL_BYTE, payload.GUARD_BYTE)
                t = ctx.copy(0, sub(dst, doff), sub(src, soff), n, iters)
                want = "copy" if iters == 1 else protocol
                assert mpx.PROTOCOLS.get(t.protocol) == want, (soff, doff, n, iters, t.protocol)
                assert t.launches == (iters if want == "copy" else 1) and t.bytes == n * iters
                assert_region(ctx, dst, doff, host[soff:soff + n],
                              what=f"{protocol} src+{soff} -> dst+{doff}, {n} B x {iters}")


def test_copy_launch_at_interior_pointers(ctx, copy_bufs, monkeypatch):
    """k_copy (a launch per copy): 16-byte aligned pointers inside an
    allocation, a tail with and without a body, more than one workgroup;
    nothing written before dst or past its end."""
    monkeypatch.setenv("MPX_COPY", "launch")
    _copies(ctx, copy_bufs, [1, 15, 16, 17, 4096 + 5, 8192 + 16 + 3], [1, 2], "copy")


@pytest.mark.parametrize("shape", [None, "2:1:1:3:1024", "64:0:0:8:256", "32:0:0:1:1024:1"])
def test_copy_steps_at_interior_pointers(ctx, copy_bufs, monkeypatch, shape):
    """k_copy_steps, its default shapes (one workgroup; one XCD) and forced
    ones, indexing from interior pointers"""
    monkeypatch.setenv("MPX_COPY", "steps" + (":" + shape if shape else ""))
    sizes = [17, (16 << 10) + 17, (128 << 10) + 33] if shape is None else [(128 << 10) + 33]
    _copies(ctx, copy_bufs, sizes, [2, 3], "copy_steps")


@pytest.mark.parametrize("hier", [0, 1])
@pytest.mark.parametrize("upl", [1, 8, 16])
def test_copy_pipe_at_interior_pointers(ctx, copy_bufs, monkeypatch, upl, hier):
    """k_copy_pipe builds its buffer resources from src / dst and the tail's
    from src + body: interior pointers, both barrier forms, 1 to 16 units
    per lane, odd and even copy counts"""
    monkeypatch.setenv("MPX_COPY", f"pipe:{upl}:{hier}")
    _copies(ctx, copy_bufs, [17, 4096 * 5 + 3, (256 << 10) + 16 + 5], [2, 3], "copy_pipe")


# --------------------------------------------------------------------------
# E. mpx_fill / mpx_checksum: alignment contract, interior pointers
# --------------------------------------------------------------------------
def test_misaligned_pointers_are_refused(ctx):
    """mpx_checksum needs a 16-byte aligned pointer, mpx_fill an 8-byte
    aligned one (include/mpx.h): MPX_ERR_INVALID before any launch"""
    buf = ctx.alloc(0, 4096)
    try:
        ctx.fill(buf, 4096, mpx.FILL_BYTE, payload.GUARD_BYTE)
        for o in (1, 4, 8):
            with pytest.raises(mpx.MpxError) as e:
                ctx.checksum(buf, 64, offset=o)
            assert e.value.status == mpx.ERR_INVALID, o
        for o in (1, 4):
            for pattern, arg in ((mpx.FILL_BYTE, 0x11), (mpx.FILL_SPLITMIX, COPY_KEY)):
                with pytest.raises(mpx.MpxError) as e:
                    ctx.fill(sub(buf, o), 64, pattern, arg)
                assert e.value.status == mpx.ERR_INVALID, o
        assert ctx.read(buf, 4096) == b"\xee" * 4096
        # nothing to touch: nothing to align
        assert ctx.checksum(buf, 0, offset=1) == O.checksum(b"")
        ctx.fill(sub(buf, 1), 0, mpx.FILL_BYTE, 0x11)
        assert ctx.read(buf, 4096) == b"\xee" * 4096
    finally:
        ctx.free(buf)


def test_checksum_of_arbitrary_bytes_at_interior_pointers(ctx):
    """k_checksum over bytes no fill kernel produced, at 16-byte aligned
    offsets inside an allocation, every tail length: the host's checksum of
    the same bytes"""
    total = 4080 + 65537
    host = np.random.default_rng(1).integers(0, 256, total, dtype=np.uint8).tobytes()
    buf = ctx.alloc(0, total)
    try:
        payload.write(ctx, buf, host)
        payload.compare(ctx.read(buf, total), host, 0, "written bytes")
        for o in (0, 16, 48, 4080):
            for n in (0, 1, 7, 8, 9, 15, 16, 17, 31, 33, 4096 + 5, 65537):
                assert ctx.checksum(buf, n, offset=o) == O.checksum(host[o:o + n]), (o, n)
    finally:
        ctx.free(buf)


@pytest.mark.parametrize("pattern,arg", [(mpx.FILL_BYTE, 0xA7), (mpx.FILL_SPLITMIX, COPY_KEY)])
def test_fill_at_interior_pointers(ctx, pattern, arg):
    """k_fill's 8-byte stores and byte tail from an 8-byte aligned interior
    pointer: the oracle's bytes, nothing before or after them"""
    total = 4088 + 4096 + 5 + GUARD
    buf = ctx.alloc(0, total)
    try:
        for o in (8, 24, 4088):
            for n in (1, 7, 8, 9, 255, 4096 + 5):
                ctx.fill(buf, total, mpx.FILL_BYTE, payload.GUARD_BYTE)
                ctx.fill(sub(buf, o), n, pattern, arg)
                assert_region(ctx, buf, o, O.fill(n, pattern, arg), what=f"fill of {n} B at +{o}")
    finally:
        ctx.free(buf)
