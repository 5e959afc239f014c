"""GPU worker for tests/test_gpu_hostlink_seq.py: sequenced host-link calls in
a process of its own, under whatever MPX_TEST knob and MPX_HOSTLINK_LL its
environment sets.

argv[1]: a JSON list of cases, each a dict
    mode, gpu_group, n, iters, check (0|1), nwg (optional)
    alt (optional): [side, index, kind, value] - that side ("gpu" | "host")
        expects, at iteration `index`, the checksum of other bytes than the
        honest payload's: kind "payload" = the peer's payload of iteration
        `value`, "tx" = the first bytes of the peer's seeded tx, "byte" = the
        byte `value` repeated
    full (optional, 1): verify the call as hostlink_seq.call does (every byte
        of both ends, every counter) and report "verified"
    rx_gpu (optional): [kind, value] - compare the GPU rank's rx afterwards
Prints one JSON line: per case each side's status and counts, the call's
protocol, and the comparisons asked for.  Every expectation is host bytes."""
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mpi-perf_amd"))
sys.path.insert(0, HERE)
import mpx  # noqa: E402
import oracle_py  # noqa: E402
import hostlink_seq as S  # noqa: E402
from seq import SEED, sent  # noqa: E402

cases = json.loads(sys.argv[1])
h = S.one(max(c["n"] for c in cases))
g, e = S.LINK


def other_bytes(kind, value, src, dst, m):
    if kind == "payload":
        return sent(SEED, src, dst, value, m)
    if kind == "tx":
        return h.tx_bytes[src][:m]
    return bytes([value]) * m


res = []
for c in cases:
    mode, gpu_group, n, iters, check = c["mode"], c["gpu_group"], c["n"], c["iters"], bool(c["check"])
    nwg = c.get("nwg", 0)
    if c.get("full"):
        out = S.call(h, mode, gpu_group, n, iters, check=check, nwg=nwg, what=str(c))
        res.append({"verified": True, "protocol": out[g].protocol, "nwg": [out[g].nwg, out[e].nwg]})
        continue
    S.prepare(h)
    want = {}
    for r, peer, group in ((g, e, gpu_group), (e, g, 1 - gpu_group)):
        want[r] = S.expectations(peer, r, S.lens(mode, group, n)[1], iters)
    if c.get("alt"):
        side, index, kind, value = c["alt"]
        r, peer = (g, e) if side == "gpu" else (e, g)
        m = S.lens(mode, gpu_group if side == "gpu" else 1 - gpu_group, n)[1]
        want[r][index] = oracle_py.checksum(other_bytes(kind, value, peer, r, m))
    out, errs = {}, {}

    def side_call(r):
        try:
            if r == g:
                out[r] = h.c.xfer_hostlink_seq(mode, gpu_group, g, e, iters, *h.gpu[g], n, SEED, check_payload=check,
                                               expect=want[r] if check else None, timeout_ms=5000, nwg=nwg)
            else:
                out[r] = h.c.host_xfer_seq(mode, 1 - gpu_group, e, g, iters, n, SEED, check_payload=check,
                                           expect=want[r] if check else None, timeout_ms=5000, nwg=nwg)
        except mpx.MpxError as x:
            errs[r] = x

    th = [threading.Thread(target=side_call, args=(r,), daemon=True) for r in (g, e)]
    for t in th:
        t.start()
    for t in th:
        t.join(S.JOIN_S)
    if any(t.is_alive() for t in th):
        print(json.dumps({"hung": c}))
        os._exit(3)
    one = {"gpu": S.record(out, errs, g), "host": S.record(out, errs, e)}
    if c.get("rx_gpu"):
        kind, value = c["rx_gpu"]
        m = S.lens(mode, gpu_group, n)[1]
        got = h.rx(g)
        exp = other_bytes(kind, value, e, g, m) + bytes([S.GUARD_BYTE]) * (h.cap - m)
        one["rx_gpu_ok"] = got == exp
        one["rx_gpu_head"] = got[:8].hex()
    res.append(one)
h.close()
print(json.dumps(res))
