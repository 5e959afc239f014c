"""CPU checks of the diagnostic tools the round-5 root cause rests on
(profiles/r05_exit_stall_symbolized.txt): tools/symbolize_frames.py names the
stripped ROCm frames of profiles/r04_procs_exit_stall.txt by the strings and
calls of their enclosing functions.  Tied to the image's ROCm 7.2 build (the
offsets are that build's): skipped on another build."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = "/opt/rocm/lib/libamdhip64.so.7"
HSA = "/opt/rocm/lib/libhsa-runtime64.so.1"
HIP_BUILD_ID = "c7eeb80a2701f2525f81fea6b13c88cc5df7013c"


def build_id(path):
    r = subprocess.run(["readelf", "-n", path], capture_output=True, text=True)
    return next((ln.split()[-1] for ln in r.stdout.splitlines() if "Build ID" in ln), None)


def symbolize(lib, *offsets):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "symbolize_frames.py"), lib, *offsets],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-400:]
    return r.stdout


@pytest.mark.skipif(not os.path.exists(HIP) or build_id(HIP) != HIP_BUILD_ID, reason="not the image's HIP build")
def test_stall_frames_are_named():
    out = symbolize(HIP, "0x3ea90f", "0x3fff31", "0x3fd4f9", "0x4b499")
    assert "Deleting CG enabled hardware queue" in out            # roc::Device::releaseQueue
    assert "There was a timestamp that was not used; deleting." in out   # ~VirtualGPU
    assert "Handler: value(%d), timestamp(%p), handle(0x%lx)" in out      # the completion handler
    assert "removeFatBinary" in out                                # the exit-time unregistration
    assert "hsa_queue_destroy@plt" in out


@pytest.mark.skipif(not os.path.exists(HSA), reason="no HSA runtime")
def test_kfd_wait_ioctl_request():
    """the event thread's ioctl request is AMDKFD_IOC_WAIT_EVENTS:
    _IOWR('K', 0x0c, 24-byte struct)"""
    req = 0xc0184b0c
    assert (req >> 30) == 3 and ((req >> 16) & 0x3fff) == 24 and ((req >> 8) & 0xff) == ord("K") and (req & 0xff) == 0x0c
    r = subprocess.run(["objdump", "-d", "--no-show-raw-insn", "--start-address=0x135700", "--stop-address=0x1357f0",
                        HSA], capture_output=True, text=True)
    if "$0xc0184b0c" not in r.stdout:
        pytest.skip("not the image's HSA build")
    assert "call" in r.stdout


# ---- tools/link_counter_control.py's peer-HBM cases, with stand-ins ---------
class _Buf:
    def __init__(self, dev, n, ptr):
        self.dev, self.n, self.ptr = dev, n, ptr


class _Ctx:
    def __init__(self, *a):
        self.k = 0

    def alloc(self, dev, n):
        self.k += 1
        return _Buf(dev, n, 0x1000 * self.k)

    def fill(self, *a):
        pass

    def attach(self, *a):
        pass

    def copy(self, *a):
        pass

    def xfer(self, *a, **k):
        pass

    def checksum(self, b, n):
        return 7      # every copy "checks"

    def free(self, b):
        pass

    def close(self):
        pass


class _Mpx:
    MODE_UNIDIR, FILL_BYTE, FILL_SPLITMIX = 2, 0, 1
    Context = _Ctx


def _counters(per_byte):
    """a stand-in counter module whose passes read `per_byte` x the control's
    known bytes for each counter (in that counter's unit)"""
    import bench
    nbytes = bench.PEER_CONTROL_BYTES * bench.PEER_CONTROL_ITERS
    unit = {"TCC_EA0_WRREQ_sum": 64, "TCC_EA0_WRREQ_64B_sum": 64, "TCC_EA0_WRREQ_DRAM_sum": 64,
            "TCC_EA0_WRREQ_WRITE_GMI_32B_sum": 32, "TCC_EA0_WRREQ_WRITE_IO_32B_sum": 32,
            "TCC_EA0_WRREQ_WRITE_DRAM_32B_sum": 32}

    class Pass:
        def __init__(self, bus, names):
            self.names = names

        def __enter__(self):
            return self

        def __exit__(self, *e):
            self.values = [per_byte.get(n, 0.0) * nbytes / unit[n] for n in self.names]
            return False

    class Counters:
        pass
    Counters.Pass = Pass
    return Counters, nbytes, unit


class _Hip:
    @staticmethod
    def hipIpcGetMemHandle(h, p):
        return 0


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "mpi-perf_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    import link_counter_control as T
    return T


@pytest.mark.parametrize("peer,per_byte,want", [
    # a store into peer HBM classified as DRAM at the sender: the subtraction
    # reads 0, the GMI 32-B counter the bytes -> 'gmi'
    (1, {"TCC_EA0_WRREQ_sum": 1.0, "TCC_EA0_WRREQ_DRAM_sum": 1.0, "TCC_EA0_WRREQ_WRITE_GMI_32B_sum": 1.0}, "gmi"),
    # peer writes not DRAM-classified: the subtraction reads them (first choice)
    (1, {"TCC_EA0_WRREQ_sum": 1.0, "TCC_EA0_WRREQ_WRITE_GMI_32B_sum": 1.0}, "subtraction"),
    # nothing reads the bytes: no formula, with the reason
    (1, {"TCC_EA0_WRREQ_sum": 0.5, "TCC_EA0_WRREQ_DRAM_sum": 0.5}, None),
    # one GPU: the code path only
    (0, {"TCC_EA0_WRREQ_sum": 1.0, "TCC_EA0_WRREQ_WRITE_GMI_32B_sum": 1.0}, None),
])
def test_link_counter_control_peer_cases_pick_the_formula(peer, per_byte, want):
    """the tool's peer-HBM cases — GPU 0 writing known
    bytes into an IPC-imported buffer of GPU 1 (a child process) and
    bench.peer_link_control's identical in-process case — report every EA
    write counter as a multiple of the bytes, and the formula is picked from
    that table."""
    T = _tool()
    counters, nbytes, unit = _counters(per_byte)
    seen = []

    def run_child(handle_hex):
        seen.append(handle_hex)
        vals = {n: per_byte.get(n, 0.0) * nbytes / u for n, u in unit.items()}
        return dict(T.summarise(dict(vals, TCC_EA0_WRREQ_64B_sum=0.0), nbytes), copy_checked=True, src_checksum=7)

    c = _Ctx()
    r = T.peer_cases(_Mpx, counters, _Hip, c, c.alloc(0, 16), "bus0", peer, run_child)
    assert len(seen) == 1 and set(r["peer_table"]) == {"peer_hbm_ipc", "peer_hbm"}
    for row in r["peer_table"].values():
        for k in ("TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_DRAM_sum", "TCC_EA0_WRREQ_WRITE_GMI_32B_sum",
                  "TCC_EA0_WRREQ_WRITE_IO_32B_sum"):
            assert row[k] == pytest.approx(per_byte.get(k, 0.0), abs=1e-4), (k, row)
        assert row["checked"] is True and set(row["formulas"]) == {"subtraction", "gmi", "io"}
    f = r["peer_formula"]
    assert f["formula"] == want, f
    if want is None:
        assert f["reason"].startswith("one GPU" if peer == 0 else "no formula")
    assert r["cases"]["copy->peer_hbm_ipc"]["copy_checked_by_owner"] is True


# ---- tools/stream_loop_check.cpp: the stream engines' loop on the CPU ---------
def test_stream_loop_on_the_cpu(tmp_path):
    """mpx_stream_loop.h compiled with plain g++ and run with a recording
    operations object: its own checks (exact sequences per engine, window
    arithmetic, publish schedule, capture equivalence) pass; the launches it
    counts, plus the call's handshake and graph replays, are the literals the
    GPU test holds the SDMA engine to (tests/stream_launches.py); and a checked
    non-blocking call accounts for the receives the compiled reference's ranks
    completed (tests/golden/ref_runs.json, the shim's recv_done per run)."""
    import shutil

    import oracle_py as O
    import stream_launches as SL

    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "stream_loop_check")
    b = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-I" + os.path.join(ROOT, "mpi-perf_amd", "csrc"),
                        os.path.join(ROOT, "tools", "stream_loop_check.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-1500:]
    p = subprocess.run([exe, "counts"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    rows = [ln.split() for ln in p.stdout.splitlines()]
    seen = set()
    for _, pull, mode, group, n, iters, check, i0, count in ([r[0]] + [int(x) for x in r[1:]] for r in rows
                                                             if r[0] == "launches"):
        replays, covered = SL.replayed(iters, bool(check))
        assert i0 == covered, (pull, mode, group, n, iters, check)
        want = SL.launches(bool(pull), mode, group, n, iters, bool(check))
        assert want == count + SL.handshake(mode, group, iters) + replays, (pull, mode, group, n, iters, check)
        seen.add((pull, mode, group, n, iters, check))
    assert len(seen) == 2 * 3 * 2 * len(SL.SIZES) * len(SL.SHAPES)     # every literal of the table
    accounted = {(r[1], int(r[2])): int(r[3]) for r in rows if r[0] == "accounted"}
    golden = {c["name"]: c for c in O.golden()["cases"]}
    for iters, per_run in [(255, 255), (256, 255), (257, 256), (512, 510), (600, 598)]:
        c = golden[f"nonblocking_window_i{iters}"]
        runs = int(c["args"][c["args"].index("-r") + 1])
        for rank in ("0", "1"):
            assert c["shim"][rank]["recv_done"] == runs * per_run
        for kind in ("pull", "nbcheck", "rccl"):
            assert accounted[(kind, iters)] * runs == c["shim"]["0"]["recv_done"], (kind, iters)
