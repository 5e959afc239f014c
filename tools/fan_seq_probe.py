"""What generating every block of a fan call (mpx_xfer_fan_seq) costs beside
the ordinary fan call that re-sends tx (mpx_xfer_fan).

N loopback ranks on GPU 0 (one host thread each, a threading barrier before
every call) run the shapes the project quotes for the fan exchange,

    bulk      4 MiB x 50, N = 4 (3 links per rank)
    LL        8 B and 4 KiB with MPX_FAN_LL, N = 2, 4, 8 (1, 3 and 7 links per
              rank), 2000 iterations

five times each as an ordinary and as a sequenced call, unchecked — the two
alternate in one job, so drift hits both alike.  One JSON line per call: the
time per iteration on the kernel's own clock (the slowest link's device_s /
iterations) and the slowest rank's wall time.  A last line per shape gives
each form's median with its minimum and maximum.  Loopback: every byte goes
HBM -> HBM inside one GPU, no link is in it; no pass mark, no headline.

    python tools/fan_seq_probe.py [--repeats 5] > profiles/fan_seq_loopback.jsonl
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

# (name, ranks, block bytes, iterations, MPX_FAN_LL)
SHAPES = [("bulk_4MiB", 4, 4 << 20, 50, False)]
SHAPES += [(f"ll_{b}B_{n - 1}links", n, b, 2000, True) for b in (8, 4096) for n in (2, 4, 8)]
SEED = 7


def one_call(c, bufs, n, b, stride, iters, ll, seq):
    out, errs = {}, []
    bar = threading.Barrier(n)

    def side(r):
        try:
            peers = [p for p in range(n) if p != r]
            bar.wait()
            if seq:
                out[r] = c.xfer_fan_seq(r, peers, iters, bufs[r][0], bufs[r][1], b, stride, SEED, timeout_ms=20000, ll=ll)
            else:
                out[r] = c.fan(r, peers, iters, bufs[r][0], bufs[r][1], b, stride, timeout_ms=20000, ll=ll)
        except Exception as e:  # noqa: BLE001
            errs.append(f"rank {r}: {e}")
            bar.abort()
    th = [threading.Thread(target=side, args=(r,)) for r in range(n)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errs:
        raise RuntimeError("; ".join(errs))
    return out


for name, n, b, iters, ll in SHAPES:
    stride = (b + 4095) & ~4095
    with mpx.Context(n, "kernel") as c:
        bufs = []
        for r in range(n):
            tx, rx = c.alloc(0, n * stride), c.alloc(0, n * stride)
            c.fill(tx, n * stride, mpx.FILL_SPLITMIX, r + 11)
            c.attach(r, 0, tx, rx, n * stride)
            bufs.append((tx, rx))
        for seq in (False, True):
            one_call(c, bufs, n, b, stride, iters, ll, seq)           # warm-up
        per = {"ordinary": [], "seq": []}
        wall = {"ordinary": [], "seq": []}
        for rep in range(args.repeats):
            for form in ("ordinary", "seq"):
                res = one_call(c, bufs, n, b, stride, iters, ll, form == "seq")
                us = max(l["device_s"] for _, links in res.values() for l in links) / iters * 1e6
                w = max(t.wall_s for t, _ in res.values()) * 1e6
                per[form].append(us)
                wall[form].append(w)
                t0 = res[0][0]
                rec = dict(shape=name, ranks=n, links_per_rank=n - 1, block_bytes=b, iters=iters, form=form, rep=rep,
                           per_iter_us=round(us, 4), wall_us=round(w, 1), nwg=t0.nwg, protocol=t0.protocol)
                if not ll:      # bytes landed by all ranks per iteration of the slowest link
                    rec["GBps_landed"] = round(n * (n - 1) * b / (us * 1e-6) / 1e9, 1)
                print(json.dumps(rec), flush=True)
        summ = dict(shape=name, ranks=n, links_per_rank=n - 1, block_bytes=b, iters=iters, summary=True,
                    repeats=args.repeats, kind="loopback (one GPU, no link in it; no pass mark, no headline)")
        for form in ("ordinary", "seq"):
            summ[form] = dict(median_us=round(statistics.median(per[form]), 4), min_us=round(min(per[form]), 4),
                              max_us=round(max(per[form]), 4), wall_median_us=round(statistics.median(wall[form]), 1),
                              wall_min_us=round(min(wall[form]), 1), wall_max_us=round(max(wall[form]), 1))
        print(json.dumps(summ), flush=True)
