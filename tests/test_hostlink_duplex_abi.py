"""The C-ABI of the host link's full-duplex loop (include/mpx_hostlink_duplex.h),
the CPU endpoint's side of it (mpi-perf_amd/csrc/mpx_hostlink.h: run_duplex),
mpx_perf's -X option and the kernel's place in the compiler's resource report —
everything that needs no GPU.  The loop itself runs in
tests/test_gpu_hostlink_duplex.py.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import mpx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
PKG = os.path.join(ROOT, "mpi-perf_amd")
PERF = os.path.join(PKG, "bin", "mpx_perf")
FUNCS = ["mpx_host_xfer_duplex", "mpx_xfer_hostlink_duplex"]


def _header_functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(mpx_[a-z_0-9]+)\s*\(", txt, flags=re.M)))


def test_symbols_declared_exported_and_bound():
    """declared in the new header only, which mpx.h includes after
    mpx_hostlink.h inside its extern "C" block; exported; bound; no ABI bump"""
    assert _header_functions(os.path.join(INC, "mpx_hostlink_duplex.h")) == FUNCS
    for other in ("mpx.h", "mpx_hostlink.h", "mpx_fan_lat.h"):
        assert not set(_header_functions(os.path.join(INC, other))) & set(FUNCS), other
    txt = open(mpx.HEADER_PATH).read()
    assert txt.index('#include "mpx_hostlink.h"') < txt.index('#include "mpx_hostlink_duplex.h"') < txt.index("#ifdef __cplusplus\n}")
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for s in FUNCS:
        assert f" T {s}\n" in dyn, s
        assert s in mpx._SIGS and s in mpx.header_symbols(os.path.join(INC, "mpx_hostlink_duplex.h")), s
        assert "fan" not in s and not s.startswith("mpx_lat_")
    assert mpx.lib().mpx_version() == 7 and mpx.ABI_VERSION == 7 and "#define MPX_ABI_VERSION 7" in txt
    assert mpx.PROTO_HOSTLINK_DUPLEX == 13 and len(mpx.PROTOCOLS) == 10
    assert hasattr(mpx.Context, "xfer_hostlink_duplex") and hasattr(mpx.Context, "host_xfer_duplex")
    # mpx_xfer_hostlink's arguments without the mode and the group
    ex = mpx._SIGS["mpx_xfer_hostlink"]
    assert mpx._SIGS["mpx_xfer_hostlink_duplex"] == (ex[0], ex[1][:1] + ex[1][3:])
    hx = mpx._SIGS["mpx_host_xfer"]
    assert mpx._SIGS["mpx_host_xfer_duplex"] == (hx[0], hx[1][:1] + hx[1][3:])
    # the blocking entry points still say where the loop lives, and still refuse it
    assert "the full-duplex loop is not built" not in open(os.path.join(INC, "mpx_hostlink.h")).read()


def test_validation_without_a_gpu():
    L = mpx.lib()
    t = mpx.Timing()
    assert L.mpx_xfer_hostlink_duplex(None, 0, 1, 1, None, None, 8, None, C.byref(t)) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()
    assert L.mpx_host_xfer_duplex(None, 1, 0, 1, 8, None, C.byref(t)) == mpx.ERR_INVALID
    # a NULL timing, with a pointer in ctx's place: refused before ctx is looked at
    dummy = C.create_string_buffer(64)
    assert L.mpx_xfer_hostlink_duplex(dummy, 0, 1, 1, None, None, 8, None, None) == mpx.ERR_INVALID
    assert L.mpx_host_xfer_duplex(dummy, 1, 0, 1, 8, None, None) == mpx.ERR_INVALID
    # (a context needs a GPU: the rank, range and buffer refusals run in tests/test_gpu_hostlink_duplex.py)


def _perf(tmp_path, args, env_extra=None):
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1",
               **(env_extra or {}))
    return subprocess.run([PERF, "-f", str(g1), "-n", "1", "-p", "1", "-l", str(tmp_path / "logs"), *args],
                          capture_output=True, text=True, env=env, timeout=60)


REFUSALS = [
    (["-X", "1", "-w", "1"], "invalid -X 1 without -H 1|2: the full-duplex loop runs between a GPU rank and its host endpoint"),
    (["-H", "1", "-X", "1", "-w", "1", "-x", "1"], "invalid -X 1 with -x 1: -X 1 alone selects the non-blocking loop on the host link"),
    (["-H", "2", "-X", "1", "-w", "1", "-u", "1"], "invalid -X 1 with -u 1: the full-duplex loop loads both directions"),
    (["-H", "2", "-X", "1", "-w", "2", "-a", "1"], "invalid -X 1 with -a 1: every GPU rank is paired with a host endpoint of its own"),
    (["-H", "1", "-X", "1", "-w", "2", "-m", "1"], "invalid -X 1 with -m 1: a fan run has no host endpoints"),
    (["-H", "1", "-X", "1", "-w", "2", "-m", "2"], "invalid -X 1 with -m 2: a fan run has no host endpoints"),
    (["-H", "1", "-X", "1", "-w", "1", "-A", "1"], "invalid -X 1 with -A 1: a host-link call cannot be armed ahead of the barrier"),
    (["-H", "2", "-X", "1", "-w", "1", "-L", "64"], "invalid -X 1 with -L 64: host-link calls are never traced by the latency recorder"),
    (["-H", "1", "-X", "1", "-w", "1", "-d", "1"], "invalid -X 1 with -d 1: the .NET launcher lines describe pairs of ranks"),
    (["-H", "1", "-X", "1", "-w", "1", "-e", "sdma"], "invalid -X 1 with -e sdma|rccl: the host link runs on the kernel engine only"),
    (["-H", "1", "-X", "1", "-w", "1", "-e", "rccl"], "invalid -X 1 with -e sdma|rccl: the host link runs on the kernel engine only"),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_mpx_perf_refuses_X_with(tmp_path, args, message):
    """a configuration error with its own line and exit status 255, before any
    GPU work (HIP_VISIBLE_DEVICES hides every device), and no log folder"""
    p = _perf(tmp_path, args)
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message + "\n" in p.stderr, p.stderr[-400:]
    assert p.stderr.count("invalid -") == 1 and "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_X_is_parsed_and_in_the_usage_text(tmp_path):
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 255
    assert p.stderr.index("-X <1: with -H, every run is the full-duplex non-blocking loop across the host link") > \
        p.stderr.index("-H <1|2: each of the -w ranks is a GPU rank paired with a CPU endpoint")
    # a bad value has a message of its own; the other options' text is as it was
    for bad in ("2", "x", "-1", ""):
        p = _perf(tmp_path, ["-H", "1", "-X", bad, "-w", "1"])
        assert p.returncode == 255 and "bad value for -X (0 or 1)\n" in p.stderr, (bad, p.stderr[-300:])
        assert "bad value for -e" not in p.stderr and not (tmp_path / "logs").exists()
    p = _perf(tmp_path, ["-H", "3", "-X", "1", "-w", "1"])
    assert p.returncode == 255 and "bad value for -e / -S / -L / -P / -H" in p.stderr
    # -X 0 is the run without it; -H 1 -X 1 with a valid job gets as far as the GPU (none visible here)
    p = _perf(tmp_path, ["-X", "0", "-H", "1", "-w", "1", "-x", "1"])
    assert p.returncode == 255 and "invalid -H 1 with -x 1" in p.stderr
    p = _perf(tmp_path, ["-H", "1", "-X", "1", "-w", "1"])
    assert "invalid" not in p.stderr and "bad value" not in p.stderr and p.returncode != 0


WINDOW_ITERS = [0, 1, 255, 256, 257, 511, 512, 600]


def test_window_arithmetic_of_the_cpu_endpoint(tmp_path):
    """run_duplex against a CPU thread in the kernel's place, in a stand-alone
    g++ program (tools/hostlink_duplex_host_check.cpp with arguments, no
    sanitizer): the receives it reports complete are the reference's, iters -
    iters // 256 (slot 255 of each full window is never waited for)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "window"
    subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tools", "hostlink_duplex_host_check.cpp"), "-o", str(exe)], check=True,
                   capture_output=True)
    p = subprocess.run([str(exe)] + [str(i) for i in WINDOW_ITERS], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-800:]
    got = [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()]
    assert got == [(i, i - i // 256) for i in WINDOW_ITERS]


def test_cpu_endpoint_under_the_host_sanitizers(tmp_path):
    """tools/asan_hostlink_duplex.sh: run_duplex against a CPU thread in the
    kernel's place, in a stand-alone program built with
    -fsanitize=address,undefined and once more with -fsanitize=thread (CPU
    only; nothing is loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_hostlink_duplex.sh"), str(tmp_path)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert p.stdout.count("hostlink_duplex_host_check: ok") == 2
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr


def test_kernel_registers_in_the_build_output(tmp_path):
    """k_hostlink_duplex in the compiler's resource report, compiled with the
    flags the Makefile builds the library with (read as
    tests/test_hostlink_abi.py reads them): no scratch, no spill, no AGPRs, at
    most 128 VGPRs, four workgroups to a CU, and no more SGPRs than the k_xfer
    family takes.  DESIGN.md §5 "Host link: full duplex" records the figures
    of the current build."""
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    mk = open(os.path.join(PKG, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, flags=re.M))
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["HIPFLAGS"]).split()
    assert "--offload-arch=gfx950" in flags and any(f.startswith("-O") for f in flags), flags
    p = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(PKG, "csrc", "mpx_kernels.hip"), "-o", str(tmp_path / "k.o")], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-1500:]
    usage = {}
    name = None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" [")[0]] = int(m.group(2))
    duplex = {k: v for k, v in usage.items() if "k_hostlink_duplex" in k}
    pair = {k: v for k, v in usage.items() if re.search(r"6k_xferILi[012]ELi[01]E", k)}
    assert len(duplex) == 1 and len(pair) == 5, (sorted(duplex), sorted(pair))
    assert not any("k_xfer_hostlink" in k for k in duplex)
    print(duplex)
    for k, v in duplex.items():
        assert v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4, (k, v)
        assert v["TotalSGPRs"] <= max(x["TotalSGPRs"] for x in pair.values()), (k, v)
