"""What the per-iteration latency recorder (mpx_lat_*) costs the loop it watches.

A loopback pair (two ranks on GPU 0, one host thread each, a threading barrier
before every call) runs the two shapes the project quotes,

    8 B ping-pong, 100 000 iterations   (the half round trip)
    4 MiB unidir,  500 iterations

`repeats` times each with tracing off and, where the library has the recorder,
on — off and on alternate, so drift hits both alike.  One JSON line per call:
the per-iteration time from the kernel's own clock (group 1's
mpx_phases.kernel_s / iterations; halved for the ping-pong half round trip),
and with tracing on the recorded distribution.  A last line per shape gives
the medians and the observer cost, on - off per iteration.

    python tools/lat_probe.py [--repeats 5] [--pkg DIR] [--label NAME]

--pkg: the mpi-perf_amd directory whose mpx package and lib/libmpx.so to use
(another build of the project, e.g. the parent commit's: "off" only there).
"""
import argparse
import json
import os
import statistics
import sys
import threading

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "mpi-perf_amd"))
ap.add_argument("--label", default="tree")
ap.add_argument("--raw-cap", type=int, default=0)
ap.add_argument("--scale", type=float, default=1.0, help="scale the iteration counts (smoke runs)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg))
import mpx  # noqa: E402

SHAPES = [("pingpong_8B", mpx.MODE_PINGPONG, 8, max(1, int(100000 * args.scale)), 0.5),
          ("unidir_4MiB", mpx.MODE_UNIDIR, 4 << 20, max(1, int(500 * args.scale)), 1.0)]
CAP = 4 << 20


def one_call(c, bufs, bar, mode, n, iters):
    out, errs = {}, []

    def side(r):
        try:
            bar.wait()
            t = c.xfer(mode, 1 - r, r, 1 - r, iters, bufs[r][0], bufs[r][1], n, timeout_ms=20000)
            out[r] = dict(c.phases(r), device_s=t.device_s)
        except Exception as e:  # noqa: BLE001
            errs.append(f"rank {r}: {e}")
            bar.abort()
    th = [threading.Thread(target=side, args=(r,)) for r in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errs:
        raise RuntimeError("; ".join(errs))
    return out


with mpx.Context(2, "kernel") as c:
    has_lat = hasattr(c, "lat_enable")
    bufs = []
    for r in range(2):
        tx, rx = c.alloc(0, CAP), c.alloc(0, CAP)
        c.fill(tx, CAP, mpx.FILL_SPLITMIX, r + 11)
        c.attach(r, 0, tx, rx, CAP)
        bufs.append((tx, rx))
    bar = threading.Barrier(2)
    for name, mode, n, iters, half in SHAPES:
        one_call(c, bufs, bar, mode, n, max(1, iters // 10))           # warm-up
        per = {"off": [], "on": []}
        for rep in range(args.repeats):
            for trace in (("off", "on") if has_lat else ("off",)):
                if has_lat:
                    for r in range(2):
                        c.lat_enable(r, args.raw_cap) if trace == "on" else c.lat_disable(r)
                ph = one_call(c, bufs, bar, mode, n, iters)
                us = ph[0]["kernel_s"] / iters * half * 1e6                 # rank 0 = group 1
                per[trace].append(us)
                rec = dict(label=args.label, shape=name, bytes=n, iters=iters, trace=trace, rep=rep,
                           per_iter_us=round(us, 4), wall_us=round(max(ph[0]["wall_s"], ph[1]["wall_s"]) * 1e6, 1))
                if mode == mpx.MODE_UNIDIR:
                    rec["GBps"] = round(n / (us * 1e-6) / 1e9, 1)
                if trace == "on":
                    for r, g in ((0, "g1"), (1, "g0")):
                        lat = c.lat_get(r)
                        rec[g] = dict(count=lat["count"], min_us=lat["min_ticks"] / 100,
                                      p50_us=mpx.lat_quantile(lat, 0.5) / 100, p99_us=mpx.lat_quantile(lat, 0.99) / 100,
                                      p999_us=mpx.lat_quantile(lat, 0.999) / 100, max_us=lat["max_ticks"] / 100,
                                      mean_us=round(lat["sum_ticks"] / max(lat["count"], 1) / 100, 4),
                                      max_iter=lat["max_iter"])
                print(json.dumps(rec), flush=True)
        summ = dict(label=args.label, shape=name, summary=True, repeats=args.repeats,
                    off_median_us=round(statistics.median(per["off"]), 4), off_min_us=round(min(per["off"]), 4),
                    off_max_us=round(max(per["off"]), 4))
        if per["on"]:
            summ.update(on_median_us=round(statistics.median(per["on"]), 4), on_min_us=round(min(per["on"]), 4),
                        on_max_us=round(max(per["on"]), 4),
                        observer_cost_ns_per_iter=round((statistics.median(per["on"]) - statistics.median(per["off"]))
                                                        / half * 1e3, 2))
        print(json.dumps(summ), flush=True)
