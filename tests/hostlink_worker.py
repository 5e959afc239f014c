"""GPU worker for tests/test_gpu_hostlink.py::test_a_lost_payload_fails_the_receivers_check:
one unidir host-link call of 5 iterations with every payload checked, then the
same call unchecked, under whatever MPX_TEST knob its environment sets (the
gate is read once per process, hence a process of its own).
argv: d2h | h2d (who sends the B-byte payloads: the GPU rank or the host
endpoint), the size.  Prints one JSON line: each side's status and counts."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mpi-perf_amd"))
sys.path.insert(0, HERE)
import mpx  # noqa: E402
from hostlink import HostLinks  # noqa: E402

direction, n = sys.argv[1], int(sys.argv[2])
gpu_group = 1 if direction == "d2h" else 0     # group 1 sends the payloads
h = HostLinks(n)
sender, receiver = (0, 1) if direction == "d2h" else (1, 0)


def record(out, errs, r):
    t = errs[r].timing if r in errs else out[r]
    return {"status": errs[r].status if r in errs else mpx.OK, "check_failures": t.check_failures,
            "check_iters": t.check_iters, "recv_done": t.recv_done}


out, errs = h.run(mpx.MODE_UNIDIR, gpu_group, n, 5, check=True, timeout_ms=5000)
res = {"sender": record(out, errs, sender), "receiver": record(out, errs, receiver)}
out, errs = h.run(mpx.MODE_UNIDIR, gpu_group, n, 5, check=False, timeout_ms=5000)
res["unchecked"] = [errs[r].status if r in errs else mpx.OK for r in (0, 1)]
h.close()
print(json.dumps(res))
