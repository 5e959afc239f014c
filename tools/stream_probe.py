"""Host cost of the SDMA engine's enqueue loop: wall_s / iters of a loopback pair.

Two ranks on GPU 0 (tests/pairs.py), the four shapes that cover the engine's
host paths:

    ping-pong 8 B x 15                 plain enqueue, about 3 operations per iteration
    ping-pong 8 B x 600                graph replay
    non-blocking 4096 B x 600, check   the checked window, the longest plainly enqueued loop
    pulled ping-pong 65541 B x 15      the pull form

33 calls each, the first 3 dropped; one JSON line per shape with the median
and the minimum of the slower rank's wall_s / iters (us) and both ranks'
launches.  To compare two builds, run it on each in one job on one box,
alternating, with MPX_LIB naming the other build's libmpx.so:

    python tools/stream_probe.py [--label NAME] [--reading K]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpi-perf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("MPX_TEST", "")
import mpx  # noqa: E402
from pairs import Pairs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="tree")
ap.add_argument("--reading", type=int, default=1)
args = ap.parse_args()

SHAPES = [("pingpong_8B_x15", mpx.MODE_PINGPONG, 8, 15, False, False),
          ("pingpong_8B_x600", mpx.MODE_PINGPONG, 8, 600, False, False),
          ("nonblocking_4096B_x600_check", mpx.MODE_NONBLOCKING, 4096, 600, True, False),
          ("pull_pingpong_65541B_x15", mpx.MODE_PINGPONG, 65541, 15, False, True)]
P = Pairs("sdma", 1, 65541, fill="seeded")
try:
    for name, mode, n, iters, check, pull in SHAPES:
        vals = []
        for k in range(33):
            out, errs = P.run(mode, n, iters, check=check, pull=pull)
            assert not errs, errs
            if k >= 3:
                vals.append(max(out[r].wall_s for r in (0, 1)) / iters * 1e6)
        print(json.dumps({"tree": args.label, "reading": args.reading, "shape": name, "calls": len(vals),
                          "us_per_iter_median": round(statistics.median(vals), 3),
                          "us_per_iter_min": round(min(vals), 3), "launches": [out[0].launches, out[1].launches]}),
              flush=True)
finally:
    P.close()
