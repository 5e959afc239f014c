"""CPU tests of tests/payload.py: the chunk arithmetic of the byte-exact GPU
cases, the checksum's blindness under a constant fill, and the comparison
that replaces it (tests/test_gpu_bytes.py runs them on the device)."""
import os
import re

import pytest

import mpx
import oracle_py as O
import payload

KEY = mpx.pattern_key(mpx.PATTERN_SEED, 0, 0, 0)


def test_min_push_chunk_is_the_librarys():
    """chunk_shape narrows with the constant run_kernel narrows with"""
    src = open(os.path.join(mpx.PKG_ROOT, "csrc", "mpx_internal.h")).read()
    m = re.search(r"constexpr long long kMinPushChunk = (\d+);", src)
    assert m and int(m.group(1)) == payload.MIN_PUSH_CHUNK


@pytest.mark.parametrize("case", sorted(payload.EDGE_CASES))
def test_edge_cases_have_the_claimed_chunks(case):
    """every (nwg, n) of the empty / tail-only chunk test is the shape it is
    there for, by the code's own arithmetic"""
    nwg, n = case
    width, chunk, empty, last, its = payload.chunk_shape(nwg, n)
    assert (width, chunk, empty, last, its) == payload.EDGE_CASES[case]
    # what the numbers mean, from first principles: chunk_of's [lo, hi)
    assert chunk % 16 == 0 and width == min(nwg, -(-n // 1024))
    spans = [(w * chunk, min(w * chunk + chunk, n)) for w in range(width)]
    assert sum(max(hi - lo, 0) for lo, hi in spans) == n
    assert [w for w, (lo, hi) in enumerate(spans) if lo >= hi] == list(range(width - empty, width))
    assert spans[last][1] == n and spans[last][1] - spans[last][0] == its
    assert last == width - empty - 1


def test_edge_cases_cover_what_they_are_for():
    C = payload.EDGE_CASES
    assert C[(256, 456131)][2] == 1 and C[(256, 456131)][4] % 16 == 3        # one empty, tail 3
    assert {C[k][2] for k in C} == {0, 1, 3}                                  # no, one, several empty
    assert C[(65, 66561)][4] == 1                                             # a tail and no unit
    assert C[(256, (1 << 20) + 1)][4] == 17                                   # one unit + 1
    assert C[(256, 262145)][4] == 65                                          # units + 1


def test_the_suites_earlier_cases_have_no_empty_workgroup():
    """why the cases above were added: none of the nine earlier width cases
    has a workgroup with lo >= n"""
    earlier = [(1, 40000), (1, 70001), (7, 456131), (8, 456131), (33, (1 << 20) + 17), (128, (4 << 20) + 3),
               (256, (20 << 20) + 5), (64, 20000), (256, 3000)]
    assert all(payload.chunk_shape(nwg, n)[2] == 0 for nwg, n in earlier)


def test_chunk_shape_small_and_zero():
    assert payload.chunk_shape(256, 0) == (1, 0, 1, -1, 0)
    assert payload.chunk_shape(256, 1) == (1, 16, 0, 0, 1)
    assert payload.chunk_shape(256, 3000) == (3, 1008, 0, 2, 984)
    assert payload.chunk_shape(1, 70001) == (1, 70016, 0, 0, 70001)


def _swap_words(b: bytes, i: int, j: int) -> bytes:
    x = bytearray(b)
    x[8 * i:8 * i + 8], x[8 * j:8 * j + 8] = b[8 * j:8 * j + 8], b[8 * i:8 * i + 8]
    return bytes(x)


def _move_unit(b: bytes, i: int, j: int) -> bytes:
    """16-byte unit i taken out and put back in at unit position j"""
    units = [b[k:k + 16] for k in range(0, len(b) - len(b) % 16, 16)]
    u = units.pop(i)
    units.insert(j, u)
    return b"".join(units) + b[len(b) - len(b) % 16:]


def _dup_word(b: bytes, i: int, j: int) -> bytes:
    """word i delivered twice, word j never"""
    x = bytearray(b)
    x[8 * j:8 * j + 8] = b[8 * i:8 * i + 8]
    return bytes(x)


@pytest.mark.parametrize("n", [2045, 71681])
@pytest.mark.parametrize("edit", [_swap_words, _move_unit, _dup_word])
def test_constant_fill_hides_misplacement(n, edit):
    """The reference-faithful fill (memset 'a' / 'b') makes every word equal,
    so the checksum — sum of mix64(word_k + (k + 1) G) — cannot tell a
    permuted, moved or duplicated-for-omitted delivery from the right one;
    the same edit on the seeded pattern changes it."""
    const = O.fill(n, mpx.FILL_BYTE, ord("a"))
    assert const == b"a" * n
    assert O.checksum(edit(const, 3, 100)) == O.checksum(const)
    seeded = O.fill(n, mpx.FILL_SPLITMIX, KEY)
    moved = edit(seeded, 3, 100)
    assert len(moved) == n and moved != seeded
    assert O.checksum(moved) != O.checksum(seeded)


def test_seeded_prefix_is_the_shorter_fill():
    """tests fill a pair's whole capacity once and expect O.fill(n) in rx"""
    whole = O.fill(70001, mpx.FILL_SPLITMIX, KEY)
    for n in (0, 1, 7, 8, 9, 2045, 66561):
        assert whole[:n] == O.fill(n, mpx.FILL_SPLITMIX, KEY)


def _flip(b: bytes, i: int) -> bytes:
    x = bytearray(b)
    x[i] ^= 0x01
    return bytes(x)


@pytest.mark.parametrize("n", [1, 17, 4096 + 5])
def test_compare_finds_every_kind_of_damage(n):
    expect = O.fill(n, mpx.FILL_SPLITMIX, KEY)
    size = 200 + n + 64
    start, want = payload.region(200, expect, size)
    assert (start, len(want)) == (136, n + 128)
    assert want[:64] == want[-64:] == b"\xee" * 64 and want[64:64 + n] == expect
    payload.compare(want, want, start)                      # equal: silent
    spots = {"first byte": 64, "last byte": 64 + n - 1, "first guard byte": 0, "guard byte before": 63,
             "guard byte after": 64 + n, "last guard byte": len(want) - 1}
    if n > 16:
        spots["16-byte boundary"] = 64 + 16
        spots["byte before the boundary"] = 64 + 15
    for name, i in spots.items():
        with pytest.raises(AssertionError) as e:
            payload.compare(_flip(want, i), want, start, name)
        msg = str(e.value)
        assert f"first at offset {start + i} " in msg and f"1 of {len(want)} bytes differ" in msg, (name, msg)
        assert "got " in msg and "want " in msg


def test_compare_reports_count_and_context():
    want = bytes(range(64))
    got = bytearray(want)
    got[20:24] = b"\xff\xff\xff\xff"
    with pytest.raises(AssertionError) as e:
        payload.compare(bytes(got), want, 1000, "rx of rank 1")
    msg = str(e.value)
    assert msg.startswith("rx of rank 1: 4 of 64 bytes differ, first at offset 1020 (last at 1023)")
    assert "bytes [1012, 1028)" in msg
    assert "got " + bytes(got[12:28]).hex(" ") in msg and "want " + want[12:28].hex(" ") in msg
    with pytest.raises(AssertionError):
        payload.compare(want[:-1], want)


def test_region_front_guard_is_cut_at_the_buffer_start():
    assert payload.region(0, b"ab", 66) == (0, b"ab" + b"\xee" * 64)
    assert payload.region(8, b"ab", 74) == (0, b"\xee" * 8 + b"ab" + b"\xee" * 64)
    with pytest.raises(AssertionError):
        payload.region(0, b"ab", 65)                        # the rear guard must fit


def test_sub_buffer():
    b = mpx.Buffer(0x7f0000001000, 0, 4096)
    s = payload.sub(b, 48)
    assert (s.ptr, s.dev, s.size) == (b.ptr + 48, 0, 4048)


# ---- the wrap points of tests/test_gpu_wrap.py, on the host ------------------
WRAP_CPP = r"""#include "mpx_internal.h"
#include <cstdio>
using namespace mpx;
int main() {
    unsigned long long a, b, c;
    char op[16];
    while (scanf("%15s %llu %llu %llu", op, &a, &b, &c) == 4) {
        if (op[0] == 't') printf("%u\n", ll_tag(a));
        else if (op[0] == 'f') printf("%llu\n", fin_word(a, b, b, b, b, b, b, c));
        else if (op[0] == 's') printf("%d\n", ring_slots(a, (long long)b));
        else printf("%d\n", ring_slot((int)a, (int)b, (int)c));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def internal(tmp_path_factory):
    """mpx_internal.h's own host functions, through a host-only program (the
    way tests/test_abi.py compiles the completion line): lines of "op a b c"
    in, one number per line out"""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("wrap")
    (d / "wrap.cpp").write_text(WRAP_CPP)
    subprocess.run([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                    os.path.join(mpx.PKG_ROOT, "csrc"), str(d / "wrap.cpp"), "-o", str(d / "wrap")],
                   check=True, capture_output=True)

    def ask(rows):
        text = "".join(f"{op} {a} {b} {c}\n" for op, a, b, c in rows)
        out = subprocess.run([str(d / "wrap")], input=text, check=True, capture_output=True, text=True).stdout.split()
        assert len(out) == len(rows)
        return [int(x) for x in out]
    return ask


P31, P32 = 1 << 31, 1 << 32


def test_ll_tag_is_never_zero_and_wraps_at_2_31_exactly(internal):
    """ll_tag's contract (mpx_internal.h): never 0, so a zeroed mailbox never
    matches; distinct for pushes 1 .. 2^31 - 1 apart; EQUAL at a distance of
    exactly 2^31 — the documented bound, which
    tests/test_gpu_wrap.py is written around"""
    bases = [1, 2, P31 - 4, P31 - 1, P31, P31 + 1, P32 - 4, P32 - 1, P32, P32 + 1, 3 * P31 - 1, (1 << 63) + 5,
             (1 << 64) - P31 - 1]
    near = [1, 2, 3, 4, 8, 9, 255, 256, (1 << 16), (1 << 30), P31 - 2, P31 - 1]
    rows = [("t", s, 0, 0) for s in bases] + [("t", s + d, 0, 0) for s in bases for d in near + [P31]]
    tags = internal(rows)
    assert all(0x80000000 <= t <= 0xFFFFFFFF for t in tags)
    base, rest = tags[:len(bases)], tags[len(bases):]
    for k, s in enumerate(bases):
        mine = rest[k * (len(near) + 1):(k + 1) * (len(near) + 1)]
        assert all(t != base[k] for t in mine[:-1]), s
        assert mine[-1] == base[k], s
        assert len(set(mine[:-1])) == len(near), s
    # the run the GPU cases cross: pushes 2^31 - 1, 2^31, 2^31 + 1, and push 1
    assert internal([("t", P31 - 1, 0, 0), ("t", P31, 0, 0), ("t", P31 + 1, 0, 0), ("t", 1, 0, 0)]) == [
        0xFFFFFFFF, 0x80000000, 0x80000001, 0x80000001]


def test_a_cleared_completion_line_is_never_a_sealed_one(internal):
    """tokens 2^32 and 2^33 have a low word of 0, like the line launch_call
    clears: the seal of seven zero fields is not 0, so fin_sealed rejects the
    cleared line (and any all-equal line the test tries)"""
    for token in (P32, 2 * P32, 3 * P32):
        words = internal([("f", token, v, v) for v in (0, 1, token)])
        assert all(w != 0 and w & 0xFFFFFFFF == 0 and w >> 32 != 0 for w in words), (token, words)
        assert len(set(words)) == 3


def test_ring_arithmetic_is_the_librarys(internal):
    """payload.ring_slots / ring_slot restate mpx_internal.h; the credit case
    of tests/test_gpu_wrap.py (three slots for 4097-byte messages) rests on
    them and on ring_bytes_for"""
    cases = [(0, 4097), (8322, 4097), (8193, 4097), (12291, 4097), (64 << 20, 1), (64 << 20, 0), (255 * 4161, 4097)]
    assert internal([("s", rb, n, 0) for rb, n in cases]) == [payload.ring_slots(rb, n) for rb, n in cases]
    assert payload.ring_slots(payload.ring_bytes_for(4097 + payload.GUARD, 2 * (4097 + payload.GUARD)), 4097) == 3
    assert payload.ring_bytes_for(4161, 0) == 0 and payload.ring_bytes_for(4161) == 255 * 4161
    assert payload.ring_bytes_for(1 << 20) == 64 << 20
    # 20 receives in 3 slots: the last lands in rx (slot 0), each slot is reused
    slots = internal([("r", j, 20, 3) for j in range(20)])
    assert slots == [(19 - j) % 3 for j in range(20)] and slots[-1] == 0
