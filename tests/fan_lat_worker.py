"""Child processes of tests/test_gpu_fan_lat.py (MPX_TEST is the parent's choice):

    fan_lat_worker.py lag     under MPX_TEST=lag_wg=1:0:20000
    fan_lat_worker.py wrap    under MPX_TEST=

lag: a checked 20-iteration 4096-byte LL fan call on a full mesh of 3, every
rank's link recorder on; rank 1's workgroup of link 0 (to rank 0) stalls 20 ms
between its push and its wait of iteration 10.  wrap: every link of a 3-mesh
starts 4 pushes short of 2^32 (mpx_test_advance_link), then 9 traced, checked
iterations.  Both go through Fan.checked_call (host bytes, digests, link
counters) and print one JSON line: every link's mpx_lat and raw stamps, and
every rank's wall_s.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "mpi-perf_amd"))
sys.path.insert(0, HERE)
from fan import full_mesh  # noqa: E402
from fan_ll import mesh  # noqa: E402

RAW_CAP = 64
LINKS3 = [(0, 1), (0, 2), (1, 2)]


def report(F, sets, out):
    links = {f"{r}-{p}": dict(lat=F.c.fan_lat_get(r, p), raw=F.c.fan_lat_raw(r, p)) for r in sets for p in sets[r]}
    return dict(ok=True, links=links, wall_s={str(r): out[r][0].wall_s for r in sets})


def traced_call(iters, what, before=None):
    sets = full_mesh(3)        # peers in rank order
    F = mesh(3, 4096)
    try:
        if before:
            before(F)
        for r in sets:
            F.c.fan_lat_enable(r, RAW_CAP)
        out = F.checked_call(sets, iters, True, what)
        print(json.dumps(report(F, sets, out)))
    finally:
        F.close()


def wrap_jump(F):
    for l in LINKS3:
        F.jump(l, (1 << 32) - 4)


if __name__ == "__main__":
    if sys.argv[1] == "lag":
        traced_call(20, "lag")
    else:
        traced_call(9, "wrap", before=wrap_jump)
