"""The host-link recorder's C-ABI (include/mpx_hostlink_lat.h), the CPU
endpoint's traced loop (mpi-perf_amd/csrc/mpx_hostlink.h), mpx_perf's -T option
and the traced kernels' registers — everything that needs no GPU.  The
recorder itself runs in tests/test_gpu_hostlink_lat.py.
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
FUNCS = ["mpx_hostlink_lat_disable", "mpx_hostlink_lat_enable", "mpx_hostlink_lat_get", "mpx_hostlink_lat_raw",
         "mpx_hostlink_lat_reset"]
HOSTLINK_FUNCS = ["mpx_host_attach", "mpx_host_buffers", "mpx_host_checksum", "mpx_host_xfer", "mpx_hostlink_ll_max",
                  "mpx_xfer_hostlink"]


def _header_functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(mpx_[a-z_0-9]+)\s*\(", txt, flags=re.M)))


def test_symbols_declared_exported_and_bound(tmp_path):
    assert _header_functions(os.path.join(INC, "mpx_hostlink_lat.h")) == FUNCS
    # declared by including mpx.h alone: a C11 translation unit that takes their addresses
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "decl.c"
    src.write_text('#include "mpx.h"\n'
                   "int (*const f_enable)(mpx_ctx *, int, int) = mpx_hostlink_lat_enable;\n"
                   "int (*const f_disable)(mpx_ctx *, int) = mpx_hostlink_lat_disable;\n"
                   "int (*const f_reset)(mpx_ctx *, int) = mpx_hostlink_lat_reset;\n"
                   "int (*const f_get)(mpx_ctx *, int, int, mpx_lat *) = mpx_hostlink_lat_get;\n"
                   "int (*const f_raw)(mpx_ctx *, int, int, uint64_t *, int, int *) = mpx_hostlink_lat_raw;\n"
                   "_Static_assert(MPX_HOSTLINK_LAT_RAW_MAX == 65536, \"raw max\");\n"
                   "_Static_assert(MPX_ABI_VERSION == 7, \"abi\");\n")
    p = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", INC, "-c", str(src), "-o", str(tmp_path / "decl.o")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-1500:]
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for s in FUNCS:
        assert f" T {s}\n" in dyn, s
        assert s in mpx._SIGS, s
    assert mpx._SIGS["mpx_hostlink_lat_enable"] == mpx._SIGS["mpx_fan_lat_enable"]
    assert mpx._SIGS["mpx_hostlink_lat_get"] == mpx._SIGS["mpx_fan_lat_get"]
    assert mpx._SIGS["mpx_hostlink_lat_raw"] == mpx._SIGS["mpx_fan_lat_raw"]
    for m in ("enable", "disable", "reset", "get", "raw"):
        assert hasattr(mpx.Context, "hostlink_lat_" + m), m


def test_header_and_abi():
    assert mpx.HOSTLINK_LAT_RAW_MAX == 65536
    hdr = open(os.path.join(INC, "mpx_hostlink_lat.h")).read()
    assert "#define MPX_HOSTLINK_LAT_RAW_MAX (1 << 16)" in hdr
    assert '#error "include mpx.h' in hdr                            # the sub-headers' guard
    # part of mpx.h, inside its extern "C" block, after the full-duplex header
    txt = open(mpx.HEADER_PATH).read()
    assert txt.index('#include "mpx_hostlink.h"') < txt.index('#include "mpx_hostlink_duplex.h"') < \
        txt.index('#include "mpx_hostlink_lat.h"') < txt.index("#ifdef __cplusplus\n}")
    # no ABI bump and no new protocol: callers detect the feature by symbol
    assert mpx.lib().mpx_version() == 7 and mpx.ABI_VERSION == 7 and "#define MPX_ABI_VERSION 7" in txt
    assert len(mpx.PROTOCOLS) == 10 and mpx.PROTO_HOSTLINK_LL == 11 and mpx.PROTO_HOSTLINK_BULK == 12
    # mpx_hostlink.h declares what it declared, and points here
    link_hdr = os.path.join(INC, "mpx_hostlink.h")
    assert _header_functions(link_hdr) == HOSTLINK_FUNCS
    assert "mpx_hostlink_lat.h" in open(link_hdr).read()
    # the endpoint's header is still plain C++ with no HIP include
    ep = open(mpx.HOSTLINK_HEADER_PATH).read()
    assert "#include <hip" not in ep and "hip_runtime" not in ep and "struct LatRec" in ep


def test_null_context():
    L = mpx.lib()
    lat = mpx.Lat()
    n = C.c_int(0)
    buf = (C.c_uint64 * 4)()
    assert L.mpx_hostlink_lat_enable(None, 0, 16) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()
    assert L.mpx_hostlink_lat_disable(None, 0) == mpx.ERR_INVALID
    assert L.mpx_hostlink_lat_reset(None, 0) == mpx.ERR_INVALID
    assert L.mpx_hostlink_lat_get(None, 0, 1, C.byref(lat)) == mpx.ERR_INVALID
    assert L.mpx_hostlink_lat_raw(None, 0, 1, buf, 4, C.byref(n)) == mpx.ERR_INVALID


def test_endpoint_recorder_under_the_host_sanitizers(tmp_path):
    """tools/asan_hostlink_lat.sh: the endpoint's traced loop against a CPU
    thread in the kernel's place — every block recomputed from its raw deltas,
    the raw cap, accumulation and reset, the host_lag knob, an untraced call
    between traced ones — in a stand-alone program built with
    -fsanitize=address,undefined and once more with -fsanitize=thread (CPU
    only; nothing is loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no C++ compiler")
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_hostlink_lat.sh"), str(tmp_path)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert p.stdout.count("hostlink_lat_host_check: ok") == 2
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr


# ---- mpx_perf -T ---------------------------------------------------------------------------------
def _perf(tmp_path, args):
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([PERF, "-f", str(g1), "-n", "1", "-p", "1", "-l", str(tmp_path / "logs"), *args],
                          capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("cap", ["64", "0", "65536"])
def test_T_with_H_passes_validation(tmp_path, cap):
    """what fails is the hidden GPU, not the option"""
    p = _perf(tmp_path, ["-H", "1", "-w", "1", "-T", cap])
    assert "invalid" not in p.stderr and "bad value" not in p.stderr and p.returncode != 0, p.stderr[-400:]


@pytest.mark.parametrize("args,message", [
    (["-w", "2", "-T", "64"], "invalid -T 64 without -H: the host-link recorder traces host-link calls only"),
    (["-H", "1", "-X", "1", "-w", "1", "-T", "64"],
     "invalid -T 64 with -X 1: the full-duplex loop is never traced by the host-link recorder"),
])
def test_mpx_perf_refuses_T(tmp_path, args, message):
    """its own line and exit status 255, before any GPU work, and no log folder"""
    p = _perf(tmp_path, args)
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message + "\n" in p.stderr, p.stderr[-400:]
    assert p.stderr.count("invalid -T") == 1 and "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


@pytest.mark.parametrize("bad", ["-1", "x", "65537"])
def test_a_bad_T_value_has_a_message_of_its_own(tmp_path, bad):
    p = _perf(tmp_path, ["-H", "1", "-w", "1", "-T", bad])
    assert p.returncode == 255 and "bad value for -T" in p.stderr, p.stderr[-400:]
    assert "bad value for -e / -S / -L / -P / -H" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_the_existing_texts_stay(tmp_path):
    p = _perf(tmp_path, ["-H", "2", "-w", "1", "-L", "64"])
    assert p.returncode == 255
    assert "invalid -H 2 with -L 64: host-link calls are never traced by the latency recorder\n" in p.stderr
    p = _perf(tmp_path, ["-H", "3", "-w", "1"])
    assert p.returncode == 255 and "bad value for -e / -S / -L / -P / -H" in p.stderr
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 255
    assert p.stderr.index("-T <raw-cap: with -H") > p.stderr.index("-X <1: with -H") > \
        p.stderr.index("-H <1|2: each of the -w ranks") > p.stderr.index("-P <raw-cap: with -m 2") > \
        p.stderr.index("-m <1: every run is one fan exchange")
    assert p.stderr.rstrip().splitlines()[-1].lstrip().startswith("-T <raw-cap")   # after every existing line


# ---- registers -----------------------------------------------------------------------------------
def test_traced_kernel_registers_in_the_build_output(tmp_path):
    """k_hostlink_lat's four instantiations in the compiler's resource report,
    compiled with the flags the Makefile builds the library with: the budget
    the untraced family is held to (128 VGPRs, no scratch, no AGPRs, no spill,
    4 waves per SIMD, no more SGPRs than the k_xfer family), and names that
    the untraced family's count (tests/test_hostlink_abi.py) does not see.  No
    count is fixed here; DESIGN.md §5 records the figures of the current build."""
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    mk = open(os.path.join(PKG, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", mk, flags=re.M))
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["HIPFLAGS"]).split()
    assert "--offload-arch=gfx950" in flags and any(f.startswith("-O") for f in flags), flags
    p = subprocess.run([hipcc, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(PKG, "csrc", "mpx_kernels.hip"), "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-1500:]
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs|VGPRs Spill): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" [")[0]] = int(m.group(2))
    traced = {k: v for k, v in usage.items() if "k_hostlink_lat" in k}
    pair = {k: v for k, v in usage.items() if re.search(r"6k_xferILi[02]ELi[01]E", k)}
    assert len(traced) == 4 and len(pair) == 4, (sorted(traced), sorted(pair))
    assert not any("k_xfer_hostlink" in k for k in traced)
    # the untraced four, and nothing else under their name (the body is inlined, not reported)
    assert len([k for k in usage if "k_xfer_hostlink" in k]) == 4
    assert not any("hostlink_body" in k for k in usage)
    print(traced)
    for k, v in traced.items():
        assert v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4, (k, v)
    assert max(v["TotalSGPRs"] for v in traced.values()) <= max(v["TotalSGPRs"] for v in pair.values())
