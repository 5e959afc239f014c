"""The fan soak's plan (tools/fan_soak.py plan(), pure Python; no GPU): for the
seeds and the step count tests/test_gpu_fan_soak.py runs, every step is a call
the library accepts and that stays co-resident, both ends of every link agree
on its width, and the steps together contain everything the soak lists — so
the soak cannot quietly miss a block length, an iteration count or a loop."""
import importlib.util
import os

import pytest

import mpx
from fan import fan_width

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def soak():
    spec = importlib.util.spec_from_file_location("fan_soak", os.path.join(ROOT, "tools", "fan_soak.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


S = soak()
NRANKS = 4


@pytest.mark.parametrize("seed", S.SUITE_SEEDS)
def test_every_step_is_a_valid_call(seed):
    steps = S.plan(S.SUITE_STEPS, seed, NRANKS)
    assert len(steps) == S.SUITE_STEPS and len({s["key"] for s in steps}) == len(steps)
    cap = S.capacity(NRANKS)
    for k, s in enumerate(steps):
        if s["kind"] == "pair":
            assert 0 <= s["a"] < s["b"] < NRANKS and s["iters"] >= 1 and s["n"] + S.GUARD <= cap, (k, s)
            continue
        peers = s["peers"]
        assert peers, (k, s)
        for r, mine in peers.items():
            assert mine and len(set(mine)) == len(mine) and r not in mine, (k, s)
            assert all(0 <= p < NRANKS and r in peers.get(p, []) for p in mine), (k, "not symmetric", s)
        n, stride = s["n"], s["stride"]
        assert 0 <= n <= stride and stride % 16 == 0, (k, s)
        assert (max(peers) + 1) * stride <= cap - S.GUARD, (k, s)
        # both ends of a link compute the same width: the library's rule takes the world size, the block
        # length, the device relation and the call's option, none of which differs between the ends (their
        # peer counts do: a hub and a leaf), and the plan gives a step one length and one option
        assert mpx.fan_width(NRANKS, n, True, s["nwg"]) == fan_width(NRANKS, n, nwg=s["nwg"]) >= 1, (k, s)
        grids = {r: len(mine) * fan_width(NRANKS, n, nwg=s["nwg"]) for r, mine in peers.items()}
        assert max(grids.values()) <= 256, (k, grids)
        assert sum(grids.values()) <= 128 * NRANKS, (k, grids)       # the default rule's own bound


@pytest.mark.parametrize("seed", S.SUITE_SEEDS)
def test_the_steps_cover_what_the_soak_lists(seed):
    steps = S.plan(S.SUITE_STEPS, seed, NRANKS)
    fan = [s for s in steps if s["kind"] == "fan"]
    pair = [s for s in steps if s["kind"] == "pair"]
    assert {s["n"] for s in fan} >= set(S.BLOCK_LENS)
    assert any(s["n"] not in S.BLOCK_LENS for s in fan)
    assert {s["iters"] for s in fan} == set(S.FAN_ITERS)
    assert {s["nwg"] for s in fan} == set(S.NWGS)
    assert {s["check"] for s in fan} == {True, False} and {s["stream"] for s in fan} == {True, False}
    assert any(s["iters"] == 0 and s["check"] for s in fan)
    assert any(s["iters"] == 64 and s["check"] for s in fan)
    assert any(s["stride"] > ((s["n"] + 15) & ~15) for s in fan) and any(s["stride"] == ((s["n"] + 15) & ~15) for s in fan)
    assert any(len(s["peers"]) < NRANKS for s in fan)                    # a rank skips a step
    assert any(len(s["peers"]) == NRANKS and all(len(v) == NRANKS - 1 for v in s["peers"].values()) for s in fan)
    assert {s["mode"] for s in pair} == set(S.PAIR_MODES)
    assert {s["n"] for s in pair} >= {0, 8, 2045}


def test_the_plan_is_a_function_of_its_seed():
    assert S.plan(40, 3) == S.plan(40, 3) != S.plan(40, 4)
