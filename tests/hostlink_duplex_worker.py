"""GPU worker for tests/test_gpu_hostlink_duplex.py: full-duplex host-link calls
in a process of its own, under whatever MPX_TEST / MPX_NB_PUBLISH its
environment sets (both are read once per process).
argv: publish        600 iterations of 4161 B at width 3, unchecked then checked,
                     verified here against host bytes (an assertion ends the worker)
      lost <n>       5 iterations checked, then the same call unchecked: each
                     side's status and counts
      lost_bytes <n> one unchecked iteration: does the byte comparison of each
                     end's rx raise?
Prints one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mpi-perf_amd"))
sys.path.insert(0, HERE)
import mpx  # noqa: E402
import payload  # noqa: E402
import hostlink_duplex as D  # noqa: E402

what = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4161
h = D.one_gpu(n)
link = h.links[0]
g, e = link


def record(out, errs, r):
    t = errs[link, r].timing if (link, r) in errs else out[link, r]
    return {"status": errs[link, r].status if (link, r) in errs else mpx.OK, "check_failures": t.check_failures,
            "check_iters": t.check_iters, "recv_done": t.recv_done}


res = {}
if what == "publish":
    done = []
    for check in (False, True):
        out = D.call(h, [link], n, 600, check=check, nwg=3, what=("publish", check))
        done += [t.recv_done for t in out.values()]
    res = {"ok": True, "recv_done": done}
elif what == "lost":
    h.reset_rx()
    out, errs = D.run(h, [link], n, 5, check=True)
    res = {"gpu": record(out, errs, g), "host": record(out, errs, e)}
    h.reset_rx()
    out, errs = D.run(h, [link], n, 5, check=False)
    res["unchecked"] = [errs[link, r].status if (link, r) in errs else mpx.OK for r in link]
elif what == "lost_bytes":
    h.reset_rx()
    out, errs = D.run(h, [link], n, 1, check=False)
    res = {"status": [errs[link, r].status if (link, r) in errs else mpx.OK for r in link], "raised": []}
    for r, peer in ((g, e), (e, g)):
        try:
            payload.compare(h.rx(r), D.want_rx(h, peer, n, 1), 0, f"rank {r}")
            res["raised"].append(False)
        except AssertionError:
            res["raised"].append(True)
else:
    raise SystemExit(f"unknown worker mode {what}")
h.close()
print(json.dumps(res))
