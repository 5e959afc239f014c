"""What generating every iteration's payload (mpx_xfer_seq) costs beside the
ordinary call that re-sends tx (mpx_xfer_ex).

A loopback pair (two ranks on GPU 0, one host thread each, a threading barrier
before every call) runs the shapes the project quotes,

    8 B ping-pong, 2000 iterations      (the half round trip)
    4 MiB unidir, 50 iterations
    4 MiB non-blocking, 50 iterations
    456131 B unidir, 10 iterations      (run-hbv3's message)

five times each as an ordinary and as a sequenced call, unchecked — the two
alternate, so drift hits both alike.  One JSON line per call: the
per-iteration time from the kernel's own clock (group 1's
mpx_phases.kernel_s / iterations; halved for the ping-pong half round trip)
and the slower side's wall time.  A last line per shape gives each form's
median with its minimum and maximum.  Loopback: no link in it, no pass mark.

    python tools/seq_probe.py [--repeats 5] > profiles/seq_loopback.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import threading

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-perf_amd"))
import mpx  # noqa: E402

SHAPES = [("pingpong_8B", mpx.MODE_PINGPONG, 8, 2000, 0.5),
          ("unidir_4MiB", mpx.MODE_UNIDIR, 4 << 20, 50, 1.0),
          ("nonblocking_4MiB", mpx.MODE_NONBLOCKING, 4 << 20, 50, 1.0),
          ("unidir_456131B", mpx.MODE_UNIDIR, 456131, 10, 1.0)]
CAP = 4 << 20


def one_call(c, bufs, bar, mode, n, iters, seq):
    out, errs = {}, []

    def side(r):
        try:
            bar.wait()
            args_ = (mode, 1 - r, r, 1 - r, iters, bufs[r][0], bufs[r][1], n)
            t = c.xfer_seq(*args_, 7, timeout_ms=20000) if seq else c.xfer(*args_, timeout_ms=20000)
            out[r] = dict(c.phases(r), nwg=t.nwg, protocol=t.protocol)
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
    bufs = []
    for r in range(2):
        tx, rx = c.alloc(0, CAP), c.alloc(0, CAP)
        c.fill(tx, CAP, mpx.FILL_SPLITMIX, r + 11)
        c.attach(r, 0, tx, rx, CAP)
        bufs.append((tx, rx))
    bar = threading.Barrier(2)
    for name, mode, n, iters, half in SHAPES:
        for seq in (False, True):
            one_call(c, bufs, bar, mode, n, iters, seq)           # warm-up
        per = {"ordinary": [], "seq": []}
        wall = {"ordinary": [], "seq": []}
        for rep in range(args.repeats):
            for form in ("ordinary", "seq"):
                ph = one_call(c, bufs, bar, mode, n, iters, form == "seq")
                us = ph[0]["kernel_s"] / iters * half * 1e6                 # rank 0 = group 1
                w = max(ph[0]["wall_s"], ph[1]["wall_s"]) * 1e6
                per[form].append(us)
                wall[form].append(w)
                rec = dict(shape=name, bytes=n, iters=iters, form=form, rep=rep, per_iter_us=round(us, 4),
                           wall_us=round(w, 1), nwg=ph[0]["nwg"], protocol=ph[0]["protocol"])
                if n >= 1 << 16:
                    rec["GBps"] = round(n * (2 if mode == mpx.MODE_NONBLOCKING else 1) / (us * 1e-6) / 1e9, 1)
                print(json.dumps(rec), flush=True)
        summ = dict(shape=name, bytes=n, iters=iters, summary=True, repeats=args.repeats)
        for form in ("ordinary", "seq"):
            summ[form] = dict(median_us=round(statistics.median(per[form]), 4), min_us=round(min(per[form]), 4),
                              max_us=round(max(per[form]), 4), wall_median_us=round(statistics.median(wall[form]), 1),
                              wall_min_us=round(min(wall[form]), 1), wall_max_us=round(max(wall[form]), 1))
        print(json.dumps(summ), flush=True)
