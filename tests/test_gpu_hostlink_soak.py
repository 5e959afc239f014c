"""A seeded sequence soak of the host link (-m gpu): GPU ranks 0 and 1 on GPU
0, host endpoints 2 and 3, links (0, 2) and (1, 3), 2 seeds x 100 steps from
tests/hostlink.py's soak_plan (tests/test_hostlink_soak_plan.py asserts the
mix on the CPU).  A step is a host-link call on one link or on both at once —
either mode, either orientation, one of eight sizes, 0 to 9 iterations, one
of three widths, checked or not — or a blocking pair call between the two GPU
ranks, which use the same tx / rx, scratch words, status line and token.
Before every step one rank's tx is drawn anew.  Every step compares the whole
rx and tx of all four ranks with host bytes and every counter of every rank
towards every rank with what the step adds (LinkMap.counted_moves).
"""
import pytest

import mpx
from hostlink import SOAK_GPU, SOAK_HOST, SOAK_LINKS, SOAK_SEEDS, LinkMap, soak_plan

pytestmark = pytest.mark.gpu

T = mpx.hostlink_ll_max()


@pytest.mark.parametrize("seed", SOAK_SEEDS)
def test_seeded_sequence(seed):
    h = LinkMap(71681, 4, SOAK_GPU, SOAK_HOST, SOAK_LINKS)
    try:
        for s in soak_plan(seed, ll_max=T):
            what = f"seed {seed} step {s['step']}: {s}"
            h.set_tx(s["reseed"], seed + s["step"] + 1)
            if s["kind"] == "pair":
                a, b = (0, 1) if s["gpu_group"] else (1, 0)
                h.pair(a, b, s["mode"], s["n"], s["iters"], check=s["check"], what=what)
                continue
            links = {"a": SOAK_LINKS[:1], "b": SOAK_LINKS[1:], "both": SOAK_LINKS}[s["kind"]]
            out = h.call(links, s["mode"], s["gpu_group"], s["n"], s["iters"], check=s["check"], nwg=s["nwg"], what=what)
            assert len(out) == 2 * len(links), what
    finally:
        h.close()
