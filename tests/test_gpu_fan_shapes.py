"""Fan exchange at the shapes tests/test_gpu_fan.py leaves out (-m gpu, MI355X;
loopback ranks on GPU 0, every expectation host bytes, tests/fan.py):

* iteration counts around the publish schedule (a flag every nb_publish() = 16
  pushes and at the last: 15, 16, 17, 32, 33);
* chunks of 256 KiB and 512 KiB per workgroup (many trips of push_units_aux
  and of the strided checksum loop; tests/test_gpu_fan.py stays at 16 KiB);
* the node's shape, eight ranks with seven links each on one GPU, at the
  default widths — 1008 workgroups at 456131 bytes, the most the default rule
  makes co-resident;
* calls that move nothing, in check mode;
* the knobs read once per process, in a child (tests/fan_knob_worker.py).
"""
import os
import sys

import pytest

import mpx
import payload
from fan import Fan, fan_width, full_mesh, round16
from payload import chunk_shape
from proc import run_bounded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("check", [True, False])
def test_publish_schedule(check):
    """without check mode (i + 1) % 16 == 0 is true once at 16 and 17, twice at
    32 and 33 and never at 15; in check mode every push publishes and every
    push from the second on waits for a credit"""
    n = 4097
    sets = full_mesh(3)
    F = Fan(3, 3 * round16(n) + payload.GUARD)
    try:
        F.layout(n, round16(n))
        for iters in (15, 16, 17, 32, 33):
            F.set_tx_seed(iters)
            F.checked_call(sets, iters, check, ("publish", iters, check), widths=fan_width(3, n))
    finally:
        F.close()


BIG = [pytest.param(1, 262144 + 17, id="1x256KiB"), pytest.param(2, (1 << 20) + 1, id="2x512KiB")]


@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("nwg,n", BIG)
def test_large_chunks(nwg, n, nranks, check):
    """one workgroup moves 256 KiB + 17 bytes (a unit and a 1-byte tail past
    the last whole trip), two move 512 KiB + 16 and 512 KiB - 15"""
    if nwg == 2:
        assert chunk_shape(2, n) == (2, (512 << 10) + 16, 0, 1, (512 << 10) - 15)
    else:
        assert chunk_shape(1, n) == (1, 262144 + 32, 0, 0, n)
    sets = full_mesh(nranks)
    F = Fan(nranks, nranks * round16(n) + payload.GUARD)
    try:
        F.layout(n, round16(n))
        out = F.checked_call(sets, 2, check, ("large chunks", nwg, n, nranks, check), widths=nwg, nwg=nwg)
        assert all(out[r][0].nwg == nwg for r in sets)
    finally:
        F.close()


@pytest.mark.parametrize("n,width", [(65555, 5), (456131, 18)])
def test_mesh8_default_widths(n, width):
    """28 pairs on one GPU, every rank listing its seven peers in another
    rotation; default widths only (5 per link: 280 workgroups; 18 = 128 // 7
    per link: 8 x 7 x 18 = 1008, all of which must be resident together)"""
    assert fan_width(8, n) == mpx.fan_width(8, n) == width and 8 * 7 * width <= 1024
    sets = {r: [(r + 1 + j) % 8 for j in range(7)] for r in range(8)}
    assert len({tuple(v) for v in sets.values()}) == 8
    F = Fan(8, 8 * round16(n) + payload.GUARD)
    try:
        F.layout(n, round16(n))
        out = F.checked_call(sets, 2, True, ("mesh8", n), widths=width)
        assert all(out[r][0].nwg == width and [l["nwg"] for l in out[r][1]] == [width] * 7 for r in sets)
    finally:
        F.close()


def test_calls_that_move_nothing_in_check_mode():
    """iters = 0 with check on (no number taken, nothing checked, rx keeps its
    prefill) and block_len = 0 with check on for 17 iterations (every chunk
    empty: it still publishes, credits and counts), then a call that moves
    bytes"""
    n = 4097
    sets = full_mesh(3)
    F = Fan(3, 3 * round16(n) + payload.GUARD)
    try:
        F.layout(n, round16(n))
        F.checked_call(sets, 0, True, "iters 0, first call of the context", widths=fan_width(3, n))
        F.checked_call(sets, 3, True, "after iters 0", widths=fan_width(3, n))
        F.checked_call(sets, 0, True, "iters 0", widths=fan_width(3, n))
        F.layout(0, 16)
        F.checked_call(sets, 17, True, "17 empty checked pushes", widths=1)
        F.layout(0, 0)
        F.checked_call(sets, 17, True, "17 empty checked pushes at stride 0", widths=1)
        F.layout(n, round16(n))
        F.checked_call(sets, 3, True, "after the empty calls", widths=fan_width(3, n))
    finally:
        F.close()


KNOBS = [pytest.param({"MPX_NB_PUBLISH": "1", "MPX_SYNC": "event"}, id="publish1-event"),
         pytest.param({"MPX_NB_PUBLISH": "256", "MPX_FAN_WG": "7"}, id="publish256-wg7"),
         pytest.param({"MPX_NB_PUBLISH": "2"}, id="publish2")]


@pytest.mark.parametrize("knobs", KNOBS)
def test_env_knobs(knobs):
    """MPX_NB_PUBLISH, MPX_FAN_WG and MPX_SYNC meet fan calls in a fresh child
    (tests/fan_knob_worker.py: host-byte verification, link counters, the
    width of every link asserted on the call's result, tokens across 2^32)"""
    env = dict(os.environ, **knobs)
    p = run_bounded([sys.executable, os.path.join(HERE, "fan_knob_worker.py")], env=env, timeout=100)
    assert p.returncode == 0 and p.stdout.split()[-1:] == ["ok"], (p.stdout[-400:], p.stderr[-1500:])
