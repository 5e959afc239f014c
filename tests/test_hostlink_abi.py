"""The host link's C-ABI (include/mpx_hostlink.h), its CPU endpoint
(mpi-perf_amd/csrc/mpx_hostlink.h) and mpx_perf's -H option — everything that
needs no GPU.  The link itself runs in tests/test_gpu_hostlink.py.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import mpx
import oracle_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
PKG = os.path.join(ROOT, "mpi-perf_amd")
PERF = os.path.join(PKG, "bin", "mpx_perf")
FUNCS = ["mpx_host_attach", "mpx_host_buffers", "mpx_host_checksum", "mpx_host_xfer", "mpx_hostlink_ll_max",
         "mpx_xfer_hostlink"]


def _header_functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(mpx_[a-z_0-9]+)\s*\(", txt, flags=re.M)))


def test_symbols_declared_exported_and_bound():
    assert _header_functions(os.path.join(INC, "mpx_hostlink.h")) == FUNCS
    # part of mpx.h, inside its extern "C" block, after the link recorder's header
    txt = open(mpx.HEADER_PATH).read()
    assert txt.index('#include "mpx_fan_lat.h"') < txt.index('#include "mpx_hostlink.h"') < txt.index("#ifdef __cplusplus\n}")
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for s in FUNCS:
        assert f" T {s}\n" in dyn, s
        assert s in mpx._SIGS, s
    # no ABI bump: callers detect the feature by symbol
    assert mpx.lib().mpx_version() == 7 and mpx.ABI_VERSION == 7 and "#define MPX_ABI_VERSION 7" in txt
    assert mpx.PROTO_HOSTLINK_LL == 11 and mpx.PROTO_HOSTLINK_BULK == 12
    for m in ("host_attach", "host_buffers", "xfer_hostlink", "host_xfer"):
        assert hasattr(mpx.Context, m), m
    assert callable(mpx.host_checksum) and callable(mpx.hostlink_ll_max)
    assert mpx._SIGS["mpx_xfer_hostlink"] == mpx._SIGS["mpx_xfer_ex"]
    assert mpx._SIGS["mpx_host_xfer"] == (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(mpx.XferOpts), C.POINTER(mpx.Timing)])


def test_struct_layouts_match_the_headers(tmp_path):
    """HostBox / HostMailbox (csrc/mpx_hostlink.h, plain C++: g++ alone builds
    it) and mpx_xfer_opts have the binding's sizes and field offsets; a
    HostBox has the device mailbox's size (the kernels address it as one)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    mirrors = {"mpx::hostlink::HostBox": mpx.HostBox, "mpx::hostlink::HostMailbox": mpx.HostMailbox,
               "mpx_xfer_opts": mpx.XferOpts}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "mpx.h"', '#include "csrc/mpx_hostlink.h"', "int main() {"]
    for cname, py in mirrors.items():
        src.append(f'    printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            src.append(f'    printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    src += ["    return 0;", "}"]
    c = tmp_path / "layout.cpp"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    # (no HIP include path: the endpoint's header must not need one)
    subprocess.run([cxx, "-std=c++17", "-Wno-invalid-offsetof", "-I", INC, "-I", PKG, str(c), "-o",
                    str(exe)], check=True, capture_output=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        name, field, val = line.split()
        got[(name, field)] = int(val)
    for cname, py in mirrors.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert C.sizeof(mpx.XferOpts) == 32
    words = 64 * 256 * 2 + 64 * 2048 + 64 * 2          # Mailbox (mpx_internal.h): flag, credit, ll, posted, ready
    assert C.sizeof(mpx.HostBox) == 8 * words and C.sizeof(mpx.HostMailbox) == 16 * words
    hdr = open(mpx.HOSTLINK_HEADER_PATH).read()
    assert "#include <hip" not in hdr and "hip_runtime" not in hdr


@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 15, 16, 17, 4099])
def test_host_checksum_is_the_oracles(n, off):
    data = oracle_py.fill(4099 + 16, mpx.FILL_SPLITMIX, mpx.pattern_key(mpx.PATTERN_SEED, 5, 6, 7))
    buf = C.create_string_buffer(data, len(data))
    out = C.c_uint64(1)
    assert mpx.lib().mpx_host_checksum(C.c_void_p(C.addressof(buf) + off), n, C.byref(out)) == mpx.OK
    assert out.value == oracle_py.checksum(data[off:off + n])
    assert mpx.host_checksum(data, off, n) == out.value


def test_validation_without_a_gpu():
    L = mpx.lib()
    t = mpx.Timing()
    out = C.c_uint64()
    assert L.mpx_xfer_hostlink(None, 0, 1, 0, 1, 1, None, None, 8, None, C.byref(t)) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()
    assert L.mpx_host_xfer(None, 0, 0, 1, 0, 1, 8, None, C.byref(t)) == mpx.ERR_INVALID
    assert L.mpx_host_attach(None, 1, 64) == mpx.ERR_INVALID
    assert L.mpx_host_buffers(None, 1, None, None) == mpx.ERR_INVALID
    assert L.mpx_host_checksum(None, 8, C.byref(out)) == mpx.ERR_INVALID
    assert L.mpx_host_checksum(b"12345678", 8, None) == mpx.ERR_INVALID
    assert L.mpx_host_checksum(None, 0, C.byref(out)) == mpx.OK and out.value == oracle_py.checksum(b"")
    # a NULL timing, with a pointer in ctx's place: refused before ctx is looked at
    dummy = C.create_string_buffer(64)
    assert L.mpx_xfer_hostlink(dummy, 0, 1, 0, 1, 1, None, None, 8, None, None) == mpx.ERR_INVALID
    assert L.mpx_host_xfer(dummy, 0, 0, 1, 0, 1, 8, None, None) == mpx.ERR_INVALID


@pytest.mark.parametrize("value,want", [(None, 256), ("0", 0), ("1", 1), ("4096", 4096), ("8192", 8192), ("8193", 256),
                                        ("-1", 256), ("abc", 256), ("", 256), ("12x", 256)])
def test_ll_threshold_follows_the_environment(value, want):
    """MPX_HOSTLINK_LL in a child process; out-of-range values fall back to the
    default, 256 (the probe's sweep: DESIGN.md §5 "Host link")"""
    env = dict(os.environ)
    env.pop("MPX_HOSTLINK_LL", None)
    if value is not None:
        env["MPX_HOSTLINK_LL"] = value
    code = f"import sys; sys.path.insert(0, {PKG!r}); import mpx; print(mpx.hostlink_ll_max())"
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 0, p.stderr[-400:]
    assert int(p.stdout) == want


def _perf(tmp_path, args, env_extra=None):
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1",
               **(env_extra or {}))
    return subprocess.run([PERF, "-f", str(g1), "-n", "1", "-p", "1", "-l", str(tmp_path / "logs"), *args],
                          capture_output=True, text=True, env=env, timeout=60)


REFUSALS = [
    (["-H", "1", "-w", "1", "-x", "1"], {}, "invalid -H 1 with -x 1: the host link runs the ping-pong and unidir loops only"),
    (["-H", "2", "-w", "2", "-a", "1"], {}, "invalid -H 2 with -a 1: every GPU rank is paired with a host endpoint of its own"),
    (["-H", "1", "-w", "2", "-m", "1"], {}, "invalid -H 1 with -m 1: a fan run has no host endpoints"),
    (["-H", "1", "-w", "2", "-m", "2"], {}, "invalid -H 1 with -m 2: a fan run has no host endpoints"),
    (["-H", "1", "-w", "1", "-A", "1"], {}, "invalid -H 1 with -A 1: a host-link call cannot be armed ahead of the barrier"),
    (["-H", "2", "-w", "1", "-L", "64"], {}, "invalid -H 2 with -L 64: host-link calls are never traced by the latency recorder"),
    (["-H", "1", "-w", "1", "-d", "1"], {}, "invalid -H 1 with -d 1: the .NET launcher lines describe pairs of ranks"),
    (["-H", "1", "-w", "1", "-e", "sdma"], {}, "invalid -H 1 with -e sdma|rccl: the host link runs on the kernel engine only"),
    (["-H", "1", "-w", "1", "-e", "rccl"], {}, "invalid -H 1 with -e sdma|rccl: the host link runs on the kernel engine only"),
    (["-H", "1"], {"MPX_RANK": "0", "MPX_SIZE": "2", "MPX_LOCAL_RANK": "0"},
     "invalid -H 1 with one process per rank: a host endpoint lives in its GPU rank's process (threads mode)"),
    (["-H", "2", "-w", "33"], {}, "invalid -H 2 with -w 33: rank r's endpoint is rank world + r, so at most 32 ranks"),
]


@pytest.mark.parametrize("args,env_extra,message", REFUSALS)
def test_mpx_perf_refuses_H_with(tmp_path, args, env_extra, message):
    """a configuration error with its own line and exit status 255, before any
    GPU work (HIP_VISIBLE_DEVICES hides every device), and no log folder"""
    p = _perf(tmp_path, args, env_extra)
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message + "\n" in p.stderr, p.stderr[-400:]
    assert p.stderr.count("invalid -H") == 1 and "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_H_is_parsed_and_in_the_usage_text(tmp_path):
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 255
    assert p.stderr.index("-H <1|2: each of the -w ranks is a GPU rank paired with a CPU endpoint") > \
        p.stderr.index("-P <raw-cap: with -m 2") > p.stderr.index("-m <1: every run is one fan exchange")
    # a value other than 1 or 2 is a bad value; -H with a valid job gets as far as the GPU (none visible here)
    p = _perf(tmp_path, ["-H", "3", "-w", "1"])
    assert p.returncode == 255 and "bad value for -e / -S / -L / -P / -H" in p.stderr
    p = _perf(tmp_path, ["-H", "1", "-w", "1"])
    assert "invalid" not in p.stderr and p.returncode != 0


def test_cpu_endpoint_under_the_host_sanitizers(tmp_path):
    """tools/asan_hostlink.sh: the endpoint's loops against a CPU thread in the
    GPU's place, in a stand-alone program built with -fsanitize=address,undefined
    and once more with -fsanitize=thread (CPU only; nothing is loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_hostlink.sh"), str(tmp_path)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert p.stdout.count("hostlink_host_check: ok") == 2
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr


def test_kernel_registers_in_the_build_output(tmp_path):
    """k_xfer_hostlink's four instantiations in the compiler's resource report,
    compiled with the flags the Makefile builds the library with (HIPFLAGS,
    read from it): no scratch, and within what __launch_bounds__(256, 4)
    allows a workgroup that must stay co-resident four to a CU — the budget
    the k_xfer instantiations are held to (128 VGPRs).  No count is fixed here;
    DESIGN.md §5 "Host link" records the figures of the current build."""
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    mk = open(os.path.join(PKG, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, flags=re.M))
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["HIPFLAGS"]).split()
    assert "--offload-arch=gfx950" in flags and any(f.startswith("-O") for f in flags), flags
    p = subprocess.run([hipcc, *flags, "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(PKG, "csrc", "mpx_kernels.hip"), "-o",
                        str(tmp_path / "k.o")], capture_output=True, text=True, timeout=600)
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
    host = {k: v for k, v in usage.items() if "k_xfer_hostlink" in k}
    pair = {k: v for k, v in usage.items() if re.search(r"6k_xferILi[02]ELi[01]E", k)}
    assert len(host) == 4 and len(pair) == 4, (sorted(host), sorted(pair))
    print({k: v for k, v in host.items()})
    for k, v in {**host, **pair}.items():
        assert v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4, (k, v)
    # the same SGPR budget as the pair kernels: the residency rule (workgroups per CU) treats them alike
    assert max(v["TotalSGPRs"] for v in host.values()) <= max(v["TotalSGPRs"] for v in pair.values())
