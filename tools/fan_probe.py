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

--ll: the lock-step LL fan exchange (MPX_FAN_LL) instead.  Per N and per block
of 8 B, 256 B, 2 KiB and 4 KiB, one JSON line with the time per iteration
(the slowest link's device_s / iters, the kernel's own clock; iterations
chosen so that a call lasts at least 10 ms; best of `--repeats`) of

    ll_fan        every rank one LL fan call with all others
    checked_bulk  the bulk fan in check mode at the same size: the only
                  lock-step fan there was before the flag (it pays a checksum,
                  poison stores and a credit round trip per iteration)

and, once per N, the 8-byte pair ping-pong's half round trip between ranks 0
and 1.  Loopback figures as above: no link is in them, no pass mark.

    python tools/fan_probe.py --ll [--repeats 5] [--ranks 2,4,8] > profiles/fan_ll_loopback.jsonl

--ll --lat: the link recorder (mpx_fan_lat_*) on the same calls.  Per N and per
block of 8 B and 4 KiB, one JSON line with

    slowest / fastest link   (by mean) p50, p99 and max of its per-iteration
                             exchange latency, from one traced call
    observer cost            traced minus untraced time per iteration (the
                             slowest link's device_s / iters as above), the
                             same calls in the same process, alternating
                             untraced / traced, best of `--repeats` each

    python tools/fan_probe.py --ll --lat [--repeats 5] [--ranks 2,4,8] > profiles/fan_ll_lat_loopback.jsonl
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
ap.add_argument("--ll", action="store_true")
ap.add_argument("--lat", action="store_true")
args = ap.parse_args()
if args.lat and not args.ll:
    ap.error("--lat goes with --ll")
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


LL_BLOCKS = (8, 256, 2048, 4096)
LAT_BLOCKS = (8, 4096)
LL_CALL_S = 0.010


def ll_probe(n):
    """one JSON line per block size: the LL fan against the checked bulk fan"""
    stride = 4096
    with mpx.Context(n, "kernel") as c:
        bufs = []
        for r in range(n):
            tx, rx = c.alloc(0, n * stride), c.alloc(0, n * stride)
            c.fill(tx, n * stride, mpx.FILL_SPLITMIX, r + 11)
            c.attach(r, 0, tx, rx, n * stride)
            bufs.append((tx, rx))
        peers = {r: [p for p in range(n) if p != r] for r in range(n)}

        def per_iter(fn, iters):
            """the slowest link's device_s / iters of one call of every rank"""
            res = together(n, lambda r: fn(r, iters))
            return max(l["device_s"] for _, links in res.values() for l in links) / iters

        def best(fn):
            iters = 200                                                # warm-up, then the call length: a short
            for _ in range(3):                                         # call is mostly the wait for the peers' launch
                t = per_iter(fn, iters)
                if t * iters >= LL_CALL_S:
                    break
                iters = int(min(200000, max(iters, LL_CALL_S / max(t, 1e-9) * 1.2)))
            return min(per_iter(fn, iters) for _ in range(args.repeats)), iters

        def pingpong(r, iters):
            return c.xfer(mpx.MODE_PINGPONG, 1 if r == 0 else 0, r, 1 - r, iters, bufs[r][0], bufs[r][1], 8,
                          timeout_ms=20000)

        def pair_half_rtt():
            def once(iters):
                res = together(2, lambda r: pingpong(r, iters))
                return max(t.device_s for t in res.values()) / iters / 2
            iters = 200
            for _ in range(3):
                t = once(iters)
                if 2 * t * iters >= LL_CALL_S:
                    break
                iters = int(min(200000, max(iters, LL_CALL_S / max(2 * t, 1e-9) * 1.2)))
            return min(once(iters) for _ in range(args.repeats)), iters

        def ll_call(b):
            return lambda r, it: c.fan(r, peers[r], it, bufs[r][0], bufs[r][1], b, stride, timeout_ms=20000, ll=True)

        def link_us(lat):
            us = lat["tick_s"] * 1e6
            return dict(p50_us=round(mpx.lat_quantile(lat, 0.5) * us, 3), p99_us=round(mpx.lat_quantile(lat, 0.99) * us, 3),
                        max_us=round(lat["max_ticks"] * us, 3), mean_us=round(lat["sum_ticks"] * us / lat["count"], 3),
                        max_iter=lat["max_iter"])

        if args.lat:
            for b in LAT_BLOCKS:
                _, iters = best(ll_call(b))                            # (recorder off: the call length)
                un, tr = [], []
                for _ in range(args.repeats):                          # alternating: untraced, traced
                    for r in range(n):
                        c.fan_lat_disable(r)
                    un.append(per_iter(ll_call(b), iters))
                    for r in range(n):
                        c.fan_lat_enable(r, 0)                         # (resets)
                    tr.append(per_iter(ll_call(b), iters))
                # the distribution: the last traced call's, every link's
                lats = {(r, p): c.fan_lat_get(r, p) for r in range(n) for p in peers[r]}
                by_mean = sorted(lats, key=lambda k: lats[k]["sum_ticks"] / lats[k]["count"])
                for r in range(n):
                    c.fan_lat_disable(r)
                print(json.dumps(dict(
                    kind="loopback (one GPU, no link in it; no pass mark, no headline)", ranks=n, links_per_rank=n - 1,
                    block_bytes=b, repeats=args.repeats, iters=iters,
                    untraced_us_per_iter=round(min(un) * 1e6, 4), traced_us_per_iter=round(min(tr) * 1e6, 4),
                    observer_cost_us_per_iter=round((min(tr) - min(un)) * 1e6, 4),
                    untraced_range_us=[round(min(un) * 1e6, 4), round(max(un) * 1e6, 4)],
                    traced_range_us=[round(min(tr) * 1e6, 4), round(max(tr) * 1e6, 4)],
                    slowest_link=dict(rank=by_mean[-1][0], peer=by_mean[-1][1], **link_us(lats[by_mean[-1]])),
                    fastest_link=dict(rank=by_mean[0][0], peer=by_mean[0][1], **link_us(lats[by_mean[0]])))), flush=True)
            return

        half, half_iters = pair_half_rtt()
        for b in LL_BLOCKS:
            sums = {r: [c.checksum(bufs[p][0], b, r * stride) for p in peers[r]] for r in range(n)}
            ll, ll_iters = best(lambda r, it: c.fan(r, peers[r], it, bufs[r][0], bufs[r][1], b, stride, timeout_ms=20000,
                                                    ll=True))
            ck, ck_iters = best(lambda r, it: c.fan(r, peers[r], it, bufs[r][0], bufs[r][1], b, stride, timeout_ms=20000,
                                                    check_payload=True, expect=sums[r]))
            print(json.dumps(dict(
                kind="loopback (one GPU, no link in it; no pass mark, no headline)", ranks=n, links_per_rank=n - 1,
                block_bytes=b, repeats=args.repeats, ll_fan_us_per_iter=round(ll * 1e6, 3), ll_fan_iters=ll_iters,
                checked_bulk_fan_us_per_iter=round(ck * 1e6, 3), checked_bulk_fan_iters=ck_iters,
                pair_pingpong_8B_half_rtt_us=round(half * 1e6, 3), pair_pingpong_iters=half_iters)), flush=True)


if args.ll:
    for n in (int(x) for x in args.ranks.split(",")):
        ll_probe(n)
    sys.exit(0)

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
