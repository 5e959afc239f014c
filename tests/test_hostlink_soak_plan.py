"""The host-link soak's step generator (tests/hostlink.py: soak_plan) for the
two committed seeds — no GPU.  tests/test_gpu_hostlink_soak.py runs exactly
these plans; a plan that never drew a bulk unidir call, an orientation, a size
or a call without iterations would leave that untested with a green soak, so
the mix is asserted here.
"""
import pytest

import mpx
from hostlink import SOAK_SEEDS, SOAK_STEPS, SOAK_WIDTHS, soak_plan, soak_sizes

PP, UNI = mpx.MODE_PINGPONG, mpx.MODE_UNIDIR
T = 256      # the default threshold the sizes T and T + 1 are drawn around


def test_two_seeds_are_committed():
    assert len(SOAK_SEEDS) == 2 and len(set(SOAK_SEEDS)) == 2 and SOAK_STEPS == 100
    assert soak_sizes(T) == (0, 1, 8, 256, 257, 2045, 4161, 71681)


@pytest.mark.parametrize("seed", SOAK_SEEDS)
def test_the_plan_is_a_function_of_its_seed(seed):
    assert soak_plan(seed) == soak_plan(seed) and len(soak_plan(seed)) == SOAK_STEPS
    assert soak_plan(seed) != soak_plan(seed + 1)
    assert soak_plan(seed, 40) == soak_plan(seed)[:40]


@pytest.mark.parametrize("seed", SOAK_SEEDS)
def test_the_plan_reaches_every_form(seed):
    plan = soak_plan(seed, ll_max=T)
    host = [s for s in plan if s["kind"] != "pair"]
    pairs = [s for s in plan if s["kind"] == "pair"]
    moving = [s for s in host if s["iters"] > 0]
    assert {s["kind"] for s in plan} == {"a", "b", "both", "pair"}
    assert {s["n"] for s in moving} == set(soak_sizes(T))
    # both modes x both orientations, each as LL and as bulk, each checked and unchecked
    forms = {(s["mode"], s["gpu_group"], s["n"] > T) for s in moving}
    assert forms == {(m, g, b) for m in (PP, UNI) for g in (0, 1) for b in (False, True)}, forms
    assert {(s["mode"], s["gpu_group"], s["check"]) for s in moving} == {(m, g, c) for m in (PP, UNI) for g in (0, 1)
                                                                         for c in (False, True)}
    assert any(s["iters"] == 0 for s in host) and any(s["iters"] == 9 for s in host)
    assert {s["nwg"] for s in moving if s["n"] > T} == set(SOAK_WIDTHS)
    assert any(s["n"] == 71681 and s["nwg"] == 70 for s in moving)        # the empty chunk
    # pair calls: both blocking modes, LL and bulk
    assert {(s["mode"], s["n"] > 2048) for s in pairs if s["iters"] > 0} == {(m, b) for m in (PP, UNI) for b in (False, True)}
    # every kind of call follows every other kind at least once, and every rank's tx is reseeded
    kinds = [("pair" if s["kind"] == "pair" else "host") for s in plan]
    assert {(a, b) for a, b in zip(kinds, kinds[1:])} == {(a, b) for a in ("pair", "host") for b in ("pair", "host")}
    assert {s["reseed"] for s in plan} == {0, 1, 2, 3}
    # a host-link call right after a pair call on the same GPU rank, and the reverse
    assert any(a["kind"] == "pair" and b["kind"] in ("a", "both") for a, b in zip(plan, plan[1:]))
    assert any(a["kind"] in ("b", "both") and b["kind"] == "pair" for a, b in zip(plan, plan[1:]))
