"""The C-ABI of the host link's sequenced payloads (include/mpx_hostlink_seq.h),
mpx_perf's -K, the endpoint's sequenced loop under the host sanitizers and the
kernels' resource report — everything that needs no GPU.  The calls themselves
run in tests/test_gpu_hostlink_seq.py.
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
FUNCS = ["mpx_host_xfer_seq", "mpx_xfer_hostlink_seq"]


def _header_functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(mpx_[a-z_0-9]+)\s*\(", txt, flags=re.M)))


def test_symbols_declared_exported_and_bound():
    assert _header_functions(os.path.join(INC, "mpx_hostlink_seq.h")) == FUNCS
    # part of mpx.h, inside its extern "C" block, after the sequenced fan's header
    txt = open(mpx.HEADER_PATH).read()
    assert txt.index('#include "mpx_fan_seq.h"') < txt.index('#include "mpx_hostlink_seq.h"') < txt.index("#ifdef __cplusplus\n}")
    # nothing was added to the older headers
    for other in ("mpx_hostlink.h", "mpx_hostlink_duplex.h", "mpx_hostlink_lat.h", "mpx_seq.h", "mpx_fan_seq.h"):
        assert not set(FUNCS) & set(_header_functions(os.path.join(INC, other))), other
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for s in FUNCS:
        assert f" T {s}\n" in dyn, s
        assert s in mpx._SIGS, s
    # no ABI bump and no new protocol number: callers detect the feature by symbol
    assert mpx.lib().mpx_version() == 7 and mpx.ABI_VERSION == 7 and "#define MPX_ABI_VERSION 7" in txt
    assert len(mpx.PROTOCOLS) == 10
    assert hasattr(mpx.Context, "xfer_hostlink_seq") and hasattr(mpx.Context, "host_xfer_seq")
    # the ordinary calls' arguments, with mpx_seq_opts in mpx_xfer_opts' place
    for new, old in (("mpx_xfer_hostlink_seq", "mpx_xfer_hostlink"), ("mpx_host_xfer_seq", "mpx_host_xfer")):
        assert mpx._SIGS[new][0] == C.c_int and mpx._SIGS[new][1][:-2] == mpx._SIGS[old][1][:-2], new
        assert mpx._SIGS[new][1][-2:] == [C.POINTER(mpx.SeqOpts), C.POINTER(mpx.Timing)], new
    hdr = open(os.path.join(INC, "mpx_hostlink_seq.h")).read()
    for said in ("mpx_xfer_seq keeps refusing a host endpoint", "stays unsequenced", "the two sides of a call need not\n   agree"):
        assert said in hdr, said


def test_validation_without_a_gpu():
    L = mpx.lib()
    t = mpx.Timing()
    o = mpx.SeqOpts()
    dummy = C.create_string_buffer(64)
    # NULL ctx / opts / timing, with a pointer in ctx's place: refused before ctx is looked at
    assert L.mpx_xfer_hostlink_seq(None, 0, 1, 0, 1, 1, None, None, 8, C.byref(o), C.byref(t)) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()
    assert L.mpx_xfer_hostlink_seq(dummy, 0, 1, 0, 1, 1, None, None, 8, None, C.byref(t)) == mpx.ERR_INVALID
    assert L.mpx_xfer_hostlink_seq(dummy, 0, 1, 0, 1, 1, None, None, 8, C.byref(o), None) == mpx.ERR_INVALID
    assert L.mpx_host_xfer_seq(None, 0, 1, 1, 0, 1, 8, C.byref(o), C.byref(t)) == mpx.ERR_INVALID
    assert L.mpx_host_xfer_seq(dummy, 0, 1, 1, 0, 1, 8, None, C.byref(t)) == mpx.ERR_INVALID
    assert L.mpx_host_xfer_seq(dummy, 0, 1, 1, 0, 1, 8, C.byref(o), None) == mpx.ERR_INVALID


def test_the_endpoints_header_is_plain_cxx_and_the_knob_is_documented():
    hdr = open(os.path.join(PKG, "csrc", "mpx_hostlink.h")).read()
    assert "#include <hip" not in hdr and "hip_runtime" not in hdr
    assert '#include "mpx_seq.h"' in hdr and "run_seq" in hdr
    rt = open(os.path.join(PKG, "csrc", "mpx_runtime.hip")).read()
    assert "//   seq_stale=k " in rt and '"seq_stale="' in rt


def _perf(tmp_path, args):
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([PERF, "-f", str(g1), "-n", "1", "-p", "1", "-l", str(tmp_path / "logs"), *args],
                          capture_output=True, text=True, env=env, timeout=60)


REFUSALS = [
    (["-K", "1", "-w", "2"], "invalid -K 1 without -H 1|2: sequenced host-link payloads are a host-link run's (-c 3 is the pair loops')"),
    (["-K", "1", "-w", "1", "-H", "1", "-X", "1"], "invalid -K 1 with -X 1: the full-duplex loop keeps sends in flight and stays unsequenced"),
    (["-K", "1", "-w", "1", "-H", "2", "-T", "16"], "invalid -K 1 with -T 16: sequenced host-link calls are never traced by the host-link recorder"),
    (["-K", "1", "-w", "1", "-H", "1", "-c", "2"], "invalid -K 1 with -c 2: a sequenced host-link call does not send tx; -c 0|1"),
    (["-K", "2", "-w", "1", "-H", "1"], "invalid -K: its value is 0 or 1"),
    (["-K", "x", "-w", "1", "-H", "1"], "invalid -K: its value is 0 or 1"),
    (["-K", "1", "-w", "1", "-H", "1", "-c", "1", "-i", "1000", "-b", "1048576"],
     "invalid -K 1 -c 1 with -i 1000 and -b 1048576: more than 268435456 bytes of expected payloads to generate per run"),
    (["-K", "1", "-w", "1", "-H", "1", "-c", "1", "-i", "300", "-S", "1:1048576"],
     "invalid -K 1 -c 1 with -i 300 and -b 1048576: more than 268435456 bytes of expected payloads to generate per run"),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_mpx_perf_refuses_K_with(tmp_path, args, message):
    """a configuration error with its own line and exit status 255, before any
    GPU work (HIP_VISIBLE_DEVICES hides every device), and no log folder"""
    p = _perf(tmp_path, args)
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message + "\n" in p.stderr, p.stderr[-400:]
    assert p.stderr.count("invalid -K") == 1 and "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_c3_with_K_keeps_c3s_own_refusal(tmp_path):
    """-c 3 -H is refused as it always was, -K or not; -K 1 -c 3 without -H gets -K's line"""
    p = _perf(tmp_path, ["-K", "1", "-w", "1", "-H", "1", "-c", "3"])
    assert p.returncode == 255
    assert "invalid -c 3 with -H 1: a host-link call sends its tx, not sequenced payloads\n" in p.stderr
    assert "invalid -K" not in p.stderr
    p = _perf(tmp_path, ["-w", "2", "-Q", "1"])
    assert p.returncode == 255 and "invalid -Q 1 without -m: " in p.stderr


def test_K_is_in_the_usage_text_and_valid_jobs_pass_validation(tmp_path):
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    line = "-K <1: with -H 1|2, every run is a sequenced host-link call on both ends: a payload per iteration; -c 0|1>"
    assert line in p.stderr
    assert p.stderr.index("-Q <1: with -m 1|2") < p.stderr.index(line) < p.stderr.index("-H <1|2: each of the -w ranks")
    # -K 0 is no switch at all; valid -K 1 jobs get as far as the GPU (none visible here)
    for extra in (["-K", "1", "-H", "1"], ["-K", "1", "-H", "2", "-u", "1", "-c", "1"], ["-K", "0", "-H", "1", "-T", "4"],
                  ["-K", "1", "-H", "1", "-c", "1", "-i", "256", "-b", "1048576"]):
        p = _perf(tmp_path, ["-w", "1"] + extra)
        assert "invalid" not in p.stderr and p.returncode != 0, (extra, p.stderr[-400:])


def test_sequenced_endpoint_loop_under_the_host_sanitizers(tmp_path):
    """tools/hostlink_seq_host_check.cpp: a stand-alone program with its own
    main, built with -fsanitize=address,undefined, run once (CPU only; nothing
    is loaded into python).  tools/asan_hostlink_seq.sh runs it under
    ThreadSanitizer as well."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "hostlink_seq_host_check"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-pthread", "-I", os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tools", "hostlink_seq_host_check.cpp"), "-o", str(exe)], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1500:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert p.stdout == "hostlink_seq_host_check: ok\n"
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr


# The nine older host-link kernels in the parent commit's resource report
# (the commit before k_hostlink_gen existed): VGPRs, occupancy, SGPRs.  Sharing
# hostlink_body with the sequenced kernels must not have changed one of them.
PARENT = {
    "_ZN3mpx15k_xfer_hostlinkILi0ELi0EEEvNS_8XferArgsE": (98, 4, 106),
    "_ZN3mpx15k_xfer_hostlinkILi0ELi1EEEvNS_8XferArgsE": (96, 5, 106),
    "_ZN3mpx15k_xfer_hostlinkILi2ELi0EEEvNS_8XferArgsE": (82, 5, 106),
    "_ZN3mpx15k_xfer_hostlinkILi2ELi1EEEvNS_8XferArgsE": (63, 7, 106),
    "_ZN3mpx14k_hostlink_latILi0ELi0EEEvNS_8XferArgsE": (108, 4, 106),
    "_ZN3mpx14k_hostlink_latILi0ELi1EEEvNS_8XferArgsE": (106, 4, 106),
    "_ZN3mpx14k_hostlink_latILi2ELi0EEEvNS_8XferArgsE": (92, 5, 106),
    "_ZN3mpx14k_hostlink_latILi2ELi1EEEvNS_8XferArgsE": (73, 6, 106),
    "_ZN3mpx17k_hostlink_duplexENS_8XferArgsE": (69, 7, 106),
}


def test_kernel_registers_in_the_build_output(tmp_path):
    """The compiler's resource report, with the flags the Makefile builds the
    library with: exactly four k_hostlink_gen instantiations, each without
    scratch, spilled VGPRs or AGPRs, within 128 VGPRs, at four waves per SIMD
    or more and with the 48 bytes of static LDS hostlink_body documents; the
    nine older host-link kernels at the parent commit's figures; still exactly
    seven kernels with `seq` in their name; hostlink_body in no kernel's place."""
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
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs|VGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" [")[0]] = int(m.group(2))
    new = {k: v for k, v in usage.items() if "k_hostlink_gen" in k}
    assert sorted(new) == sorted("_ZN3mpx14k_hostlink_genILi%dELi%dEEEvNS_8XferArgsE" % mg for mg in ((0, 0), (0, 1), (2, 0), (2, 1)))
    print(new)
    for k, v in new.items():
        assert v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4 and v["LDS Size"] == 48, (k, v)
    old = {k: v for k, v in usage.items() if "hostlink" in k and k not in new}
    assert sorted(old) == sorted(PARENT), sorted(old)
    for k, (vgprs, occupancy, sgprs) in PARENT.items():
        v = old[k]
        assert (v["VGPRs"], v["Occupancy"], v["TotalSGPRs"]) == (vgprs, occupancy, sgprs), (k, v)
        assert v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs Spill"] == 0 and v["LDS Size"] == 48, (k, v)
    assert not [k for k in usage if "hostlink_body" in k]
    # (k_xfer_seq's five, k_xfer_seq_nbcheck and the copy tool's k_seqbase)
    assert len([k for k in usage if "seq" in k]) == 7, sorted(k for k in usage if "seq" in k)
    src = open(os.path.join(PKG, "csrc", "mpx_kernels.hip")).read()
    assert "__global__ __launch_bounds__(kBlock, 4) void k_hostlink_gen(XferArgs a)" in src
