"""A short free-running soak of the fan exchange on every run of the GPU suite
(tools/fan_soak.py): four loopback ranks on GPU 0, each running the whole
seeded plan on a thread of its own without ever joining the others — fan
steps over random symmetric peer graphs (block lengths around the unit, the
1 KiB narrowing and the chunk size, strides, 0 - 64 iterations, check on and
off, streaming stores, widths) mixed with checked pair calls on the same
links.  After every call a rank compares its whole rx and tx with host bytes
and checks every reported field and its link counters, while its peers may
already be inside the next step.  tests/test_fan_soak_plan.py holds the plan
of these seeds to covering everything the soak lists.
profiles/fan_soak.jsonl holds the long runs and the no_posted control."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _soak():
    spec = importlib.util.spec_from_file_location("fan_soak", os.path.join(ROOT, "tools", "fan_soak.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


S = _soak()


@pytest.mark.parametrize("seed", S.SUITE_SEEDS)
def test_free_running_ranks_keep_every_payload(seed):
    res = S.run(S.SUITE_STEPS, seed)
    print(res)
    assert res["failures"] == 0, res
    assert res["calls"] == res["expected_calls"] > 2 * S.SUITE_STEPS, res       # every rank ran the whole plan
