"""The host link measured: a GPU rank and a CPU endpoint across PCIe, on ONE GPU.

Rank 0 is a GPU rank on GPU 0, rank 1 a host endpoint (include/mpx_hostlink.h);
each side of a call runs on a thread of its own behind a barrier.  Unlike the
loopback figures of the other probes there IS a link in these: every payload
crosses PCIe between HBM and pinned host memory.  One JSON line per item:

    latency    8 B ping-pong half round trip, both orientations: 5 calls of
               2000 iterations after a warm-up call; median, min and max.
               The time is the GPU kernel's own clock (mpx_last_phases:
               kernel_s - posted_wait_s, so neither the launch nor the wait
               for the endpoint's thread is in it) over 2 * iters.
    bandwidth  unidir at 4 MiB in each direction, widths 1 ... 128 and the
               default width: 3 calls of 50 iterations after a warm-up, best
               and median, GB/s = bytes / the same kernel time, and as a
               fraction of PCIe Gen5 x16's 63 GB/s.  Beside it hipMemcpyAsync
               between the same pinned and device buffers (the runtime's copy
               engine), 50 copies and one synchronise under a host clock, in
               the same process.
    threshold  ping-pong half round trip at 256 B ... 8 KiB, forced LL
               (MPX_HOSTLINK_LL=8192) against forced bulk (MPX_HOSTLINK_LL=0),
               median of 5 calls of 1000 iterations; the largest size at which
               LL is not slower than bulk.
    numa       the node of the endpoint's pinned memory and of the threads'
               CPUs, and the GPU's.  Nothing is bound: the line says so.

No pass mark; nothing here is asserted anywhere.

    python tools/hostlink_probe.py > profiles/hostlink.jsonl

--duplex measures the full-duplex loop instead (include/mpx_hostlink_duplex.h)
and APPENDS its lines to profiles/hostlink_duplex.jsonl (--out), all from one
process, so the figures stand beside each other's:

    duplex            the non-blocking loop at 4 MiB x 50 iterations, best and
                      median of 3 calls after a warm-up, at per-direction
                      widths 1 ... 64 and at the default width; aggregate GB/s
                      = 2 * B * iters / the kernel's own clock (posted wait
                      excluded), per direction half of it (both directions
                      move the same bytes in the same span), and as a fraction
                      of 2 x 63 GB/s.
    unidir            the two one-direction figures at the default width, the
                      same bytes, iterations and clock.
    duplex_reference  two concurrent hipMemcpyAsync streams between the same
                      buffers, one per direction, 50 copies each and one
                      synchronise of each under a host clock: the runtime's own
                      full-duplex figure; and each stream alone.
    numa              as above.

    python tools/hostlink_probe.py --duplex

--lat measures the host-link recorder (include/mpx_hostlink_lat.h) and APPENDS
its lines to profiles/hostlink_lat.jsonl (--out), all from one process:

    lat_off           tracing off: the 8 B ping-pong half round trip, both
                      orientations (5 calls of 2000 iterations), and the 4 MiB
                      unidir rate, both directions (5 calls of 50), with the
                      library's file name (MPX_LIB: the same figures from
                      another build with the recorder's symbols).  --lat-off-only
                      stops here.
    lat_observer      traced - untraced per iteration at 8 B ping-pong and
                      4 MiB unidir, with the GPU end traced only, the endpoint
                      only, and both: 5 interleaved rounds, medians.
    lat_distribution  8 B ping-pong, 100 000 iterations x 5 calls, and 4 MiB
                      unidir x 500 x 5: both ends' p50 / p99 / p99.9 / max and
                      the iteration of the maximum per call, and whether the
                      two ends name the same iteration as the slowest.
    numa              as above.

    python tools/hostlink_probe.py --lat

--seq measures what a sequenced call costs (include/mpx_hostlink_seq.h) and
APPENDS its lines to profiles/hostlink_seq.jsonl (--out), all from one process:

    seq_cost          the sequenced call beside the ordinary call of the same
                      shape, interleaved rounds in one job: the 8 B ping-pong
                      half round trip in both orientations (5 x 2000
                      iterations) and 4 MiB unidir in each direction (5 x 50),
                      on the kernel's clock.  The host-to-device bulk figure
                      includes the endpoint's CPU writing every payload into
                      its tx before it announces it; the CPU's generation rate
                      alone is tools/hostlink_seq_host_check's `rate` line.
    numa              as above.

    python tools/hostlink_probe.py --seq
"""
import argparse
import ctypes as C
import glob
import json
import os
import statistics
import sys
import threading

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--bw-bytes", type=int, default=4 << 20)
ap.add_argument("--bw-iters", type=int, default=50)
ap.add_argument("--duplex", action="store_true", help="measure the full-duplex loop; appends to --out")
ap.add_argument("--lat", action="store_true", help="measure the host-link recorder; appends to --out")
ap.add_argument("--seq", action="store_true", help="measure the sequenced calls beside the ordinary ones; appends to --out")
ap.add_argument("--lat-off-only", action="store_true", help="with --lat: the tracing-off figures only")
ap.add_argument("--lat-iters", type=int, default=100000)
ap.add_argument("--out", default=None, help="default: profiles/hostlink_duplex.jsonl, with --lat profiles/hostlink_lat.jsonl")
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                            "hostlink_seq.jsonl" if args.seq else "hostlink_lat.jsonl" if args.lat else "hostlink_duplex.jsonl")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpi-perf_amd"))
import mpx  # noqa: E402

CAP = max(args.bw_bytes, 8192) + 4096
PCIE_SPEC_GBPS = 63.0
G, E = 0, 1
KIND = "host link (GPU 0 <-> pinned host memory over PCIe); no pass mark"
os.environ.pop("MPX_HOSTLINK_LL", None)
os.environ.pop("MPX_HOSTLINK_WG", None)

hip = C.CDLL("libamdhip64.so.7")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipDeviceSynchronize.argtypes = []
hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
hip.hipStreamSynchronize.argtypes = [C.c_void_p]
hip.hipStreamDestroy.argtypes = [C.c_void_p]
libc = C.CDLL(None, use_errno=True)

c = mpx.Context(2, "kernel")
gtx, grx = c.alloc(0, CAP), c.alloc(0, CAP)
c.fill(gtx, CAP, mpx.FILL_SPLITMIX, 11)
c.attach(G, 0, gtx, grx, CAP)
c.host_attach(E, CAP)
htx, hrx = c.host_buffers(E)
for k in range(0, CAP, 4096):
    htx[k] = k & 0xff
cpu_of = {}


def call(mode, gpu_group, n, iters, nwg=0, seed=None):
    """one call, both sides; (the GPU side's loop seconds on the kernel's clock, its Timing, the endpoint's).
    seed: both sides make the sequenced call under that seed"""
    out, errs = {}, []
    bar = threading.Barrier(2)

    def side(r):
        try:
            cpu_of[r] = libc.sched_getcpu()
            bar.wait()
            if seed is not None and r == G:
                out[r] = c.xfer_hostlink_seq(mode, gpu_group, G, E, iters, gtx, grx, n, seed, timeout_ms=20000, nwg=nwg)
            elif seed is not None:
                out[r] = c.host_xfer_seq(mode, 1 - gpu_group, E, G, iters, n, seed, timeout_ms=20000, nwg=nwg)
            elif r == G:
                out[r] = c.xfer_hostlink(mode, gpu_group, G, E, iters, gtx, grx, n, timeout_ms=20000, nwg=nwg)
            else:
                out[r] = c.host_xfer(mode, 1 - gpu_group, E, G, iters, n, timeout_ms=20000, nwg=nwg)
        except Exception as e:  # noqa: BLE001
            errs.append(f"rank {r}: {e}")
            bar.abort()
    th = [threading.Thread(target=side, args=(r,)) for r in (G, E)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errs:
        raise RuntimeError("; ".join(errs))
    ph = c.phases(G)
    return ph["kernel_s"] - ph["posted_wait_s"], out[G], out[E]


def call_duplex(n, iters, nwg=0):
    """one full-duplex call, both sides; (the GPU side's loop seconds on the kernel's clock, its Timing, the endpoint's)"""
    out, errs = {}, []
    bar = threading.Barrier(2)

    def side(r):
        try:
            cpu_of[r] = libc.sched_getcpu()
            bar.wait()
            if r == G:
                out[r] = c.xfer_hostlink_duplex(G, E, iters, gtx, grx, n, timeout_ms=20000, nwg=nwg)
            else:
                out[r] = c.host_xfer_duplex(E, G, iters, n, timeout_ms=20000, nwg=nwg)
        except Exception as e:  # noqa: BLE001
            errs.append(f"rank {r}: {e}")
            bar.abort()
    th = [threading.Thread(target=side, args=(r,)) for r in (G, E)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    if errs:
        raise RuntimeError("; ".join(errs))
    ph = c.phases(G)
    return ph["kernel_s"] - ph["posted_wait_s"], out[G], out[E]


def spread(v, scale, digits=3):
    return dict(median=round(statistics.median(v) * scale, digits), min=round(min(v) * scale, digits),
                max=round(max(v) * scale, digits))


# ---- NUMA ---------------------------------------------------------------------


def node_of_cpu(cpu):
    for d in glob.glob("/sys/devices/system/node/node[0-9]*"):
        for part in open(os.path.join(d, "cpulist")).read().strip().split(","):
            lo, _, hi = part.partition("-")
            if part and int(lo) <= cpu <= int(hi or lo):
                return int(d.rsplit("node", 1)[1])
    return None


def node_of_page(addr):
    """move_pages(2) with no target nodes: the node each page is on"""
    page = C.c_void_p(addr & ~4095)
    status = C.c_int(-1)
    rc = libc.syscall(279, 0, C.c_ulong(1), C.byref(page), None, C.byref(status), 0)
    return status.value if rc == 0 else None


# ---- the full-duplex loop (--duplex) ---------------------------------------------
def duplex_probe():
    import time
    B, IT = args.bw_bytes, args.bw_iters
    lines = []

    def emit(**kw):
        lines.append(json.dumps(dict(kind=KIND, **kw)))
        print(lines[-1], flush=True)

    clock = "kernel (s_memrealtime), posted wait excluded"
    rows = []
    for nwg in (0, 1, 2, 4, 8, 16, 32, 64):
        call_duplex(B, 5, nwg)
        res = [call_duplex(B, IT, nwg) for _ in range(3)]
        gbps = [2 * B * IT / r[0] / 1e9 for r in res]
        assert all(r[1].recv_done == IT and r[2].recv_done == IT and r[1].protocol == 13 for r in res)
        rows.append(dict(nwg_asked=nwg, nwg_per_direction=res[0][1].nwg, GBps_aggregate_best=round(max(gbps), 2),
                         GBps_aggregate_median=round(statistics.median(gbps), 2),
                         GBps_per_direction_best=round(max(gbps) / 2, 2),
                         fraction_of_2x63GBps_spec=round(max(gbps) / (2 * PCIE_SPEC_GBPS), 3)))
    swept = [r for r in rows if r["nwg_asked"]]
    best = max(swept, key=lambda r: r["GBps_aggregate_median"])
    emit(item="duplex", mode="nonblocking, full duplex", bytes=B, iters=IT, calls=3, default_width=rows[0], sweep=swept,
         best_width=best["nwg_per_direction"], clock=clock)
    uni = {}
    for gpu_group, direction in ((1, "device_to_host"), (0, "host_to_device")):
        call(mpx.MODE_UNIDIR, gpu_group, B, 5)
        res = [call(mpx.MODE_UNIDIR, gpu_group, B, IT) for _ in range(3)]
        gbps = [B * IT / r[0] / 1e9 for r in res]
        uni[direction] = max(gbps)
        emit(item="unidir", direction=direction, bytes=B, iters=IT, calls=3, nwg=res[0][1].nwg, GBps_best=round(max(gbps), 2),
             GBps_median=round(statistics.median(gbps), 2), fraction_of_63GBps_spec=round(max(gbps) / PCIE_SPEC_GBPS, 3),
             clock=clock)
    emit(item="duplex_vs_unidir", default_width_aggregate_GBps=rows[0]["GBps_aggregate_best"],
         sum_of_the_unidir_figures_GBps=round(sum(uni.values()), 2),
         aggregate_over_sum=round(rows[0]["GBps_aggregate_best"] / sum(uni.values()), 3))
    # the runtime's copy engines: one stream per direction, alone and together
    st = [C.c_void_p(), C.c_void_p()]
    for x in st:
        assert hip.hipStreamCreateWithFlags(C.byref(x), 1) == 0          # hipStreamNonBlocking
    copies = (("device_to_host", C.addressof(hrx), grx.ptr, 2, st[0]), ("host_to_device", gtx.ptr, C.addressof(htx), 1, st[1]))

    def timed(which):
        v = []
        for rep in range(4):
            hip.hipDeviceSynchronize()
            t0 = time.perf_counter()
            for _ in range(IT):
                for k in which:
                    _, dst, src, kind, stream = copies[k]
                    rc = hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), B, kind, stream)
                    assert rc == 0, rc
            for k in which:
                assert hip.hipStreamSynchronize(copies[k][4]) == 0
            if rep:
                v.append(len(which) * B * IT / (time.perf_counter() - t0) / 1e9)
        return v
    # (the host-to-device copies land in the GPU rank's tx, which is filled anew below)
    alone = {copies[k][0]: timed([k]) for k in (0, 1)}
    both = timed([0, 1])
    c.fill(gtx, CAP, mpx.FILL_SPLITMIX, 11)
    for x in st:
        hip.hipStreamDestroy(x)
    emit(item="duplex_reference", what="two concurrent hipMemcpyAsync streams, one per direction, the same pinned and device "
         "buffers", bytes=B, copies_per_direction=IT, calls=3, GBps_aggregate_best=round(max(both), 2),
         GBps_aggregate_median=round(statistics.median(both), 2),
         fraction_of_2x63GBps_spec=round(max(both) / (2 * PCIE_SPEC_GBPS), 3),
         alone_GBps_best={k: round(max(v), 2) for k, v in alone.items()},
         clock="host clock around the copies and one synchronise per stream")
    try:
        gpu_node = int(open(f"/sys/bus/pci/devices/{mpx.bus_id(0).lower()}/numa_node").read())
    except OSError:
        gpu_node = None
    emit(item="numa", binding="not controlled: no thread or allocation was bound to a node", gpu_numa_node=gpu_node,
         endpoint_tx_node=node_of_page(C.addressof(htx)), endpoint_rx_node=node_of_page(C.addressof(hrx)),
         gpu_side_thread=dict(cpu=cpu_of.get(G), node=node_of_cpu(cpu_of.get(G, -1))),
         endpoint_thread=dict(cpu=cpu_of.get(E), node=node_of_cpu(cpu_of.get(E, -1))))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


# ---- the host-link recorder (--lat) ------------------------------------------------
def lat_probe():
    B, IT = args.bw_bytes, args.bw_iters
    lines = []
    clock = "kernel (s_memrealtime), posted wait excluded"

    def emit(**kw):
        lines.append(json.dumps(dict(kind=KIND, **kw)))
        print(lines[-1], flush=True)

    # tracing off (any build of the library)
    for gpu_group in (1, 0):
        call(mpx.MODE_PINGPONG, gpu_group, 8, 2000)
        v = [call(mpx.MODE_PINGPONG, gpu_group, 8, 2000)[0] / 2000 / 2 for _ in range(args.calls)]
        emit(item="lat_off", what="8 B ping-pong half round trip", gpu_group=gpu_group, calls=args.calls, iters=2000,
             half_rtt_us=spread(v, 1e6), per_call_us=[round(x * 1e6, 3) for x in v], lib=os.path.basename(mpx.LIB_PATH), clock=clock)
    for gpu_group, direction in ((1, "device_to_host"), (0, "host_to_device")):
        call(mpx.MODE_UNIDIR, gpu_group, B, 5)
        v = [B * IT / call(mpx.MODE_UNIDIR, gpu_group, B, IT)[0] / 1e9 for _ in range(args.calls)]
        emit(item="lat_off", what="unidir rate", direction=direction, bytes=B, calls=args.calls, iters=IT,
             GBps=spread(v, 1, 2), per_call_GBps=[round(x, 2) for x in v], lib=os.path.basename(mpx.LIB_PATH), clock=clock)
    if args.lat_off_only:
        return lines

    # the observer's cost: traced - untraced per iteration, interleaved rounds
    arms = (("untraced", ()), ("gpu_traced", (G,)), ("endpoint_traced", (E,)), ("both_traced", (G, E)))
    for what, mode, gpu_group, n, iters in (("8 B ping-pong", mpx.MODE_PINGPONG, 1, 8, 2000),
                                            ("8 B ping-pong", mpx.MODE_PINGPONG, 0, 8, 2000),
                                            ("4 MiB unidir", mpx.MODE_UNIDIR, 1, B, IT),
                                            ("4 MiB unidir", mpx.MODE_UNIDIR, 0, B, IT)):
        per = {name: [] for name, _ in arms}
        call(mode, gpu_group, n, iters)
        for _ in range(5):
            for name, on in arms:
                for r in on:
                    c.hostlink_lat_enable(r, 0)
                per[name].append(call(mode, gpu_group, n, iters)[0] / iters)
                for r in on:
                    c.hostlink_lat_disable(r)
        med = {k: statistics.median(v) for k, v in per.items()}
        emit(item="lat_observer", what=what, gpu_group=gpu_group, bytes=n, iters=iters, rounds=5,
             per_iteration_us={k: spread(v, 1e6) for k, v in per.items()},
             traced_minus_untraced_us={k: round((med[k] - med["untraced"]) * 1e6, 3) for k in med if k != "untraced"},
             clock=clock)

    # the distribution itself, on both ends
    def us(lat, ticks):
        return round(ticks * lat["tick_s"] * 1e6, 3)

    for what, mode, gpu_group, n, iters in (("8 B ping-pong", mpx.MODE_PINGPONG, 1, 8, args.lat_iters),
                                            ("4 MiB unidir, device to host", mpx.MODE_UNIDIR, 1, B, 500)):
        for r in (G, E):
            c.hostlink_lat_enable(r, 0)
        call(mode, gpu_group, n, min(iters, 2000))
        per_call, agree = [], 0
        for _ in range(5):
            for r in (G, E):
                c.hostlink_lat_reset(r)
            call(mode, gpu_group, n, iters)
            row = {}
            for name, r, peer in (("gpu", G, E), ("endpoint", E, G)):
                lat = c.hostlink_lat_get(r, peer)
                row[name] = dict(count=lat["count"], min_us=us(lat, lat["min_ticks"]),
                                 p50_us=us(lat, mpx.lat_quantile(lat, 0.5)), p99_us=us(lat, mpx.lat_quantile(lat, 0.99)),
                                 p999_us=us(lat, mpx.lat_quantile(lat, 0.999)), max_us=us(lat, lat["max_ticks"]),
                                 mean_us=us(lat, lat["sum_ticks"] / max(lat["count"], 1)), max_iter=lat["max_iter"])
            agree += row["gpu"]["max_iter"] == row["endpoint"]["max_iter"]
            per_call.append(row)
        for r in (G, E):
            c.hostlink_lat_disable(r)
        emit(item="lat_distribution", what=what, gpu_group=gpu_group, bytes=n, iters=iters, calls=5,
             unit="one iteration: a round trip (ping-pong) or one payload and its ack (unidir)", per_call=per_call,
             calls_where_both_ends_name_the_same_slowest_iteration=agree,
             clocks="gpu: s_memrealtime, 10 ns ticks; endpoint: CLOCK_MONOTONIC, ns")
    try:
        gpu_node = int(open(f"/sys/bus/pci/devices/{mpx.bus_id(0).lower()}/numa_node").read())
    except OSError:
        gpu_node = None
    emit(item="numa", binding="not controlled: no thread or allocation was bound to a node", gpu_numa_node=gpu_node,
         endpoint_tx_node=node_of_page(C.addressof(htx)), endpoint_rx_node=node_of_page(C.addressof(hrx)),
         gpu_side_thread=dict(cpu=cpu_of.get(G), node=node_of_cpu(cpu_of.get(G, -1))),
         endpoint_thread=dict(cpu=cpu_of.get(E), node=node_of_cpu(cpu_of.get(E, -1))))
    return lines


# ---- sequenced calls beside ordinary ones (--seq) -----------------------------------
def seq_probe():
    B, IT = args.bw_bytes, args.bw_iters
    lines = []
    clock = "kernel (s_memrealtime), posted wait excluded"

    def emit(**kw):
        lines.append(json.dumps(dict(kind=KIND, **kw)))
        print(lines[-1], flush=True)

    shapes = (("8 B ping-pong half round trip", mpx.MODE_PINGPONG, 1, 8, 2000, "half_rtt_us"),
              ("8 B ping-pong half round trip", mpx.MODE_PINGPONG, 0, 8, 2000, "half_rtt_us"),
              ("4 MiB unidir, device to host", mpx.MODE_UNIDIR, 1, B, IT, "GBps"),
              ("4 MiB unidir, host to device (the endpoint writes every payload into tx)", mpx.MODE_UNIDIR, 0, B, IT, "GBps"))
    for what, mode, gpu_group, n, iters, unit in shapes:
        per = {"ordinary": [], "sequenced": []}
        call(mode, gpu_group, n, iters)
        call(mode, gpu_group, n, iters, seed=1)
        for k in range(args.calls):
            per["ordinary"].append(call(mode, gpu_group, n, iters)[0])
            per["sequenced"].append(call(mode, gpu_group, n, iters, seed=100 + k)[0])
        if unit == "GBps":
            fig = {name: spread([n * iters / x / 1e9 for x in v], 1, 2) for name, v in per.items()}
        else:
            fig = {name: spread([x / iters / 2 for x in v], 1e6) for name, v in per.items()}
        emit(item="seq_cost", what=what, gpu_group=gpu_group, bytes=n, iters=iters, rounds=args.calls, unit=unit, **fig,
             sequenced_over_ordinary=round(fig["sequenced"]["median"] / fig["ordinary"]["median"], 3), clock=clock)
    try:
        gpu_node = int(open(f"/sys/bus/pci/devices/{mpx.bus_id(0).lower()}/numa_node").read())
    except OSError:
        gpu_node = None
    emit(item="numa", binding="not controlled: no thread or allocation was bound to a node", gpu_numa_node=gpu_node,
         endpoint_tx_node=node_of_page(C.addressof(htx)), endpoint_rx_node=node_of_page(C.addressof(hrx)),
         gpu_side_thread=dict(cpu=cpu_of.get(G), node=node_of_cpu(cpu_of.get(G, -1))),
         endpoint_thread=dict(cpu=cpu_of.get(E), node=node_of_cpu(cpu_of.get(E, -1))))
    return lines


if args.seq:
    out_lines = seq_probe()
    c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(out_lines) + "\n")
    sys.exit(0)
if args.duplex:
    duplex_probe()
    c.close()
    sys.exit(0)
if args.lat:
    out_lines = lat_probe()
    c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(out_lines) + "\n")
    sys.exit(0)

# ---- latency ------------------------------------------------------------------
for gpu_group in (1, 0):
    call(mpx.MODE_PINGPONG, gpu_group, 8, 2000)
    v = [call(mpx.MODE_PINGPONG, gpu_group, 8, 2000)[0] / 2000 / 2 for _ in range(args.calls)]
    print(json.dumps(dict(kind=KIND, item="latency", bytes=8, mode="pingpong", gpu_group=gpu_group, calls=args.calls,
                          iters=2000, half_rtt_us=spread(v, 1e6), clock="kernel (s_memrealtime), posted wait excluded",
                          ll_threshold=mpx.hostlink_ll_max())), flush=True)

# ---- bandwidth ----------------------------------------------------------------
B, IT = args.bw_bytes, args.bw_iters
best_width = {}
for gpu_group, direction in ((1, "device_to_host"), (0, "host_to_device")):
    rows = []
    for nwg in (0, 1, 2, 4, 8, 16, 32, 64, 128):
        call(mpx.MODE_UNIDIR, gpu_group, B, 5, nwg)
        res = [call(mpx.MODE_UNIDIR, gpu_group, B, IT, nwg) for _ in range(3)]
        gbps = [B * IT / r[0] / 1e9 for r in res]
        rows.append(dict(nwg_asked=nwg, nwg=res[0][1].nwg, GBps_best=round(max(gbps), 2),
                         GBps_median=round(statistics.median(gbps), 2),
                         fraction_of_63GBps_spec=round(max(gbps) / PCIE_SPEC_GBPS, 3)))
    swept = [r for r in rows if r["nwg_asked"]]
    best = max(swept, key=lambda r: r["GBps_median"])
    best_width[direction] = best["nwg"]
    print(json.dumps(dict(kind=KIND, item="bandwidth", mode="unidir", direction=direction, bytes=B, iters=IT, calls=3,
                          default_width=rows[0], sweep=swept, best_width=best["nwg"],
                          clock="kernel (s_memrealtime), posted wait excluded")), flush=True)

# the runtime's copy engine between the same buffers
import time  # noqa: E402

for direction, dst, src, kind in (("device_to_host", C.addressof(hrx), grx.ptr, 2),
                                  ("host_to_device", grx.ptr, C.addressof(htx), 1)):
    v = []
    for rep in range(4):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        for _ in range(IT):
            rc = hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), B, kind, None)
            assert rc == 0, rc
        assert hip.hipDeviceSynchronize() == 0
        if rep:
            v.append(B * IT / (time.perf_counter() - t0) / 1e9)
    print(json.dumps(dict(kind=KIND, item="bandwidth_reference", what="hipMemcpyAsync, the same pinned and device buffers",
                          direction=direction, bytes=B, copies=IT, calls=3, GBps_best=round(max(v), 2),
                          GBps_median=round(statistics.median(v), 2),
                          fraction_of_63GBps_spec=round(max(v) / PCIE_SPEC_GBPS, 3),
                          clock="host clock around the copies and one synchronise")), flush=True)

# ---- the LL threshold ---------------------------------------------------------
sizes = [256 << k for k in range(6)]
for gpu_group in (1, 0):
    rows, chosen = [], None
    for n in sizes:
        row = dict(bytes=n)
        for name, value in (("ll", "8192"), ("bulk", "0")):
            os.environ["MPX_HOSTLINK_LL"] = value
            call(mpx.MODE_PINGPONG, gpu_group, n, 200)
            v = [call(mpx.MODE_PINGPONG, gpu_group, n, 1000)[0] / 1000 / 2 for _ in range(args.calls)]
            row[name + "_half_rtt_us"] = spread(v, 1e6)
        os.environ.pop("MPX_HOSTLINK_LL", None)
        if row["ll_half_rtt_us"]["median"] <= row["bulk_half_rtt_us"]["median"]:
            chosen = n
        rows.append(row)
    print(json.dumps(dict(kind=KIND, item="ll_threshold", mode="pingpong", gpu_group=gpu_group, calls=args.calls, iters=1000,
                          sweep=rows, largest_size_where_ll_is_not_slower=chosen, in_force=mpx.hostlink_ll_max())),
          flush=True)

try:
    gpu_node = int(open(f"/sys/bus/pci/devices/{mpx.bus_id(0).lower()}/numa_node").read())
except OSError:
    gpu_node = None
print(json.dumps(dict(kind=KIND, item="numa", binding="not controlled: no thread or allocation was bound to a node",
                      gpu_numa_node=gpu_node, endpoint_tx_node=node_of_page(C.addressof(htx)),
                      endpoint_rx_node=node_of_page(C.addressof(hrx)),
                      gpu_side_thread=dict(cpu=cpu_of.get(G), node=node_of_cpu(cpu_of.get(G, -1))),
                      endpoint_thread=dict(cpu=cpu_of.get(E), node=node_of_cpu(cpu_of.get(E, -1))),
                      best_width=best_width)), flush=True)
c.close()
