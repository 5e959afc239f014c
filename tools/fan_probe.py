"""Fan exchange against the same bytes moved as rounds of pairs, on ONE GPU.

N = 2, 4, 8 loopback ranks on GPU 0 (one host thread each, a threading barrier
before every call).  Per N:

    fan     one mpx_xfer_fan per rank: a 4 MiB block to and from each of the
            N - 1 others, 50 iterations (MPX_FAN_WG=8 at N = 8)
    rounds  the same bytes as the N - 1 circle-method rounds of pairs
            (mpx.schedule), each pair one non-blocking call of 50 iterations

best of `--repeats` (5).  One JSON line per N: the fan's wall time (the
slowest rank's), every link's device_s, and the rounds' summed wall time.

A LOOPBACK figure: every byte goes HBM -> HBM inside one GPU, no link is in
it.  It says what the two call shapes cost the GPU, sets no pass mark and
feeds no headline.

    python tools/fan_probe.py [--repeats 5] [--iters 50] [--bytes 4194304] [--ranks 2,4,8]
"""
import argparse
import json
import os
import sys
import threading

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--bytes", type=int, default=4 << 20)
ap.add_argument("--ranks", default="2,4,8")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-perf_amd"))
import mpx  # noqa: E402
from mpx.schedule import all_pairs_rounds  # noqa: E402

B, ITERS = args.bytes, args.iters
STRIDE = (B + 4095) & ~4095


def together(n, fn):
    """fn(r) on a thread per rank behind one barrier; {rank: result}"""
    out, errs = {}, []
    bar = threading.Barrier(n)

    def side(r):
        try:
            bar.wait()
            out[r] = fn(r)
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


for n in (int(x) for x in args.ranks.split(",")):
    if n >= 8:
        os.environ["MPX_FAN_WG"] = "8"
    else:
        os.environ.pop("MPX_FAN_WG", None)
    with mpx.Context(n, "kernel") as c:
        bufs = []
        for r in range(n):
            tx, rx = c.alloc(0, n * STRIDE), c.alloc(0, n * STRIDE)
            c.fill(tx, n * STRIDE, mpx.FILL_SPLITMIX, r + 11)
            c.attach(r, 0, tx, rx, n * STRIDE)
            bufs.append((tx, rx))

        def fan(r, iters=ITERS):
            return c.fan(r, [p for p in range(n) if p != r], iters, bufs[r][0], bufs[r][1], B, STRIDE, timeout_ms=20000)

        def rounds(iters=ITERS):
            total = 0.0
            for rnd in all_pairs_rounds(n):
                role = {}
                for g1, g0 in rnd:
                    role[g1], role[g0] = (1, g0), (0, g1)
                res = together(n, lambda r: c.xfer(mpx.MODE_NONBLOCKING, role[r][0], r, role[r][1], iters, bufs[r][0],
                                                   bufs[r][1], B, timeout_ms=20000))
                total += max(t.wall_s for t in res.values())
            return total

        together(n, lambda r: fan(r, 2))                               # warm-up
        rounds(2)
        best_fan, best_links, best_rounds, widths = None, None, None, None
        for _ in range(args.repeats):
            res = together(n, fan)
            wall = max(t.wall_s for t, _ in res.values())
            if best_fan is None or wall < best_fan:
                best_fan = wall
                best_links = {r: [round(l["device_s"] * 1e6, 1) for l in links] for r, (_, links) in res.items()}
                widths = sorted({l["nwg"] for _, links in res.values() for l in links})
            w = rounds()
            if best_rounds is None or w < best_rounds:
                best_rounds = w
        moved = n * (n - 1) * B * ITERS                                 # bytes landed, all ranks
        slow = max((us, r, k) for r, v in best_links.items() for k, us in enumerate(v))
        print(json.dumps(dict(
            kind="loopback (one GPU, HBM-bound, no link in it; no pass mark, no headline)",
            ranks=n, block_bytes=B, iters=ITERS, repeats=args.repeats, fan_link_widths=widths,
            fan_wg_env=os.environ.get("MPX_FAN_WG"),
            fan_wall_us=round(best_fan * 1e6, 1), fan_GBps_landed=round(moved / best_fan / 1e9, 1),
            fan_link_device_us=best_links, fan_slowest_link=dict(rank=slow[1], link=slow[2], device_us=slow[0]),
            pair_rounds=n - 1, pair_rounds_wall_us=round(best_rounds * 1e6, 1),
            pair_rounds_GBps_landed=round(moved / best_rounds / 1e9, 1))), flush=True)
