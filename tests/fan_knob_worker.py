"""GPU worker for tests/test_gpu_fan_shapes.py::test_env_knobs: mesh3 fan calls
under whatever MPX_* knobs its environment sets (MPX_NB_PUBLISH and MPX_SYNC
are read once per process, hence a process of its own; MPX_FAN_WG per call).

Sizes {17, 4097, 65555} x iterations {1, 16, 33}, check on and off, every call
verified from host bytes (tests/fan.py: rx and tx whole, digests, link
counters) and every link's width asserted on the call's own result:
MPX_FAN_WG if set, narrowed to at least 1 KiB per workgroup, else the default
rule.  Then four calls with every rank's token across 2^32 (MPX_SYNC=event:
wait_kernel's hipEventSynchronize path, then the sealed completion line whose
low half reads 0 once).  Prints "ok" or raises.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mpi-perf_amd"))
sys.path.insert(0, HERE)
import mpx  # noqa: E402
import payload  # noqa: E402
from fan import Fan, fan_width, full_mesh, round16  # noqa: E402

Q = 1 << 32
SIZES, ITERS = (17, 4097, 65555), (1, 16, 33)
ENV_WG = int(os.environ.get("MPX_FAN_WG", "0"))


def main():
    sets = full_mesh(3)
    F = Fan(3, 3 * round16(max(SIZES)) + payload.GUARD)
    try:
        seed = 0
        for n in SIZES:
            width = fan_width(3, n, env=ENV_WG)
            if ENV_WG:
                assert width == min(ENV_WG, -(-n // 1024)), (n, width)
            assert width == mpx.fan_width(3, n), (n, width)
            F.layout(n, round16(n))
            for iters in ITERS:
                for check in (True, False):
                    seed += 1
                    F.set_tx_seed(seed)
                    F.checked_call(sets, iters, check, ("knobs", n, iters, check), widths=width)
        for r in range(3):
            F.advance_token(r, Q - 3 - F.counters(r, (r + 1) % 3)["token"])
        for k, check in enumerate((True, False, True, False)):
            F.set_tx_seed(100 + k)
            F.checked_call(sets, 3, check, ("knobs, token", k), widths=fan_width(3, max(SIZES), env=ENV_WG))
            for r in range(3):
                assert F.counters(r, (r + 1) % 3)["token"] == Q - 2 + k, (k, r)
                ph = F.c.phases(r)
                assert ph["kernel_s"] > 0 and ph["wall_s"] >= 0.98 * ph["kernel_s"], (k, r, ph)
    finally:
        F.close()
    print("ok")


if __name__ == "__main__":
    main()
