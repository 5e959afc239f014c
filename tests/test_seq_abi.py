"""The C-ABI of the sequenced payloads (include/mpx_seq.h), their host side
(mpi-perf_amd/csrc/mpx_seq.h) and mpx_perf's -c 3 — everything that needs no
GPU.  The calls themselves run in tests/test_gpu_seq.py.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import mpx
import oracle_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
PKG = os.path.join(ROOT, "mpi-perf_amd")
PERF = os.path.join(PKG, "bin", "mpx_perf")
FUNCS = ["mpx_seq_expect", "mpx_xfer_seq"]


def _header_functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(mpx_[a-z_0-9]+)\s*\(", txt, flags=re.M)))


def test_symbols_declared_exported_and_bound():
    assert _header_functions(os.path.join(INC, "mpx_seq.h")) == FUNCS
    # part of mpx.h, inside its extern "C" block, after the host link's headers
    txt = open(mpx.HEADER_PATH).read()
    assert txt.index('#include "mpx_hostlink_lat.h"') < txt.index('#include "mpx_seq.h"') < txt.index("#ifdef __cplusplus\n}")
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for s in FUNCS:
        assert f" T {s}\n" in dyn, s
        assert s in mpx._SIGS, s
    # no ABI bump: callers detect the feature by symbol
    assert mpx.lib().mpx_version() == 7 and mpx.ABI_VERSION == 7 and "#define MPX_ABI_VERSION 7" in txt
    assert hasattr(mpx.Context, "xfer_seq") and callable(mpx.seq_expect)
    assert mpx._SIGS["mpx_xfer_seq"][1][:-2] == mpx._SIGS["mpx_xfer_ex"][1][:-2]
    assert mpx._SIGS["mpx_xfer_seq"][1][-2:] == [C.POINTER(mpx.SeqOpts), C.POINTER(mpx.Timing)]
    assert mpx.SEQ_AUTO_MAX == 1 << 28 and "#define MPX_SEQ_AUTO_MAX (1ull << 28)" in open(os.path.join(INC, "mpx_seq.h")).read()


def test_struct_layout_matches_the_header(tmp_path):
    """mpx_seq_opts has the binding's size and field offsets; the host side's
    header needs no HIP include (g++ alone builds it)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "mpx.h"', '#include "csrc/mpx_seq.h"', "int main() {",
           '    printf("size %zu\\n", sizeof(mpx_seq_opts));']
    for f, _ in mpx.SeqOpts._fields_:
        src.append(f'    printf("{f} %zu\\n", offsetof(mpx_seq_opts, {f}));')
    src += ["    return 0;", "}"]
    c = tmp_path / "layout.cpp"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++17", "-I", INC, "-I", PKG, str(c), "-o", str(exe)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(mpx.SeqOpts) == 32
    for f, _ in mpx.SeqOpts._fields_:
        assert int(got[f]) == getattr(mpx.SeqOpts, f).offset, f
    hdr = open(os.path.join(PKG, "csrc", "mpx_seq.h")).read()
    assert "#include <hip" not in hdr and "hip_runtime" not in hdr


@pytest.mark.parametrize("it", [0, 1, 255, 1 << 24])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 13, 4161, 65537])
def test_seq_expect_is_the_oracles(n, it):
    seed = 0x0123456789ABCDEF
    for src, dst in ((0, 1), (9, 63), (63, 63)):
        want = oracle_py.checksum(oracle_py.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(seed, src, dst, it)))
        assert mpx.seq_expect(seed, src, dst, it, n) == want, (src, dst)
    # the seed, both ranks and the iteration all matter
    base = mpx.seq_expect(seed, 2, 3, it, n)
    if n:
        assert len({base, mpx.seq_expect(seed + 1, 2, 3, it, n), mpx.seq_expect(seed, 3, 2, it, n),
                    mpx.seq_expect(seed, 2, 4, it, n), mpx.seq_expect(seed, 2, 3, it + 1, n)}) == 5


def test_validation_without_a_gpu():
    L = mpx.lib()
    t = mpx.Timing()
    o = mpx.SeqOpts()
    out = C.c_uint64()
    assert L.mpx_xfer_seq(None, 0, 1, 0, 1, 1, None, None, 8, C.byref(o), C.byref(t)) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()
    # NULL opts / timing, with a pointer in ctx's place: refused before ctx is looked at
    dummy = C.create_string_buffer(64)
    assert L.mpx_xfer_seq(dummy, 0, 1, 0, 1, 1, None, None, 8, None, C.byref(t)) == mpx.ERR_INVALID
    assert L.mpx_xfer_seq(dummy, 0, 1, 0, 1, 1, None, None, 8, C.byref(o), None) == mpx.ERR_INVALID
    assert L.mpx_seq_expect(1, 0, 1, 0, 8, None) == mpx.ERR_INVALID
    for src, dst, it in ((-1, 0, 0), (0, 64, 0), (64, 0, 0), (0, 1, -1)):
        assert L.mpx_seq_expect(1, src, dst, it, 8, C.byref(out)) == mpx.ERR_INVALID
    assert L.mpx_seq_expect(1, 0, 63, 0x7FFFFFFF, 0, C.byref(out)) == mpx.OK and out.value == oracle_py.checksum(b"")


def _perf(tmp_path, args, env_extra=None):
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1",
               **(env_extra or {}))
    return subprocess.run([PERF, "-f", str(g1), "-n", "1", "-p", "1", "-l", str(tmp_path / "logs"), *args],
                          capture_output=True, text=True, env=env, timeout=60)


REFUSALS = [
    (["-c", "3", "-w", "2", "-e", "sdma"], "invalid -c 3 with -e sdma|rccl: sequenced payloads are generated by the kernel engine only"),
    (["-c", "3", "-w", "2", "-e", "rccl"], "invalid -c 3 with -e sdma|rccl: sequenced payloads are generated by the kernel engine only"),
    (["-c", "3", "-w", "2", "-m", "1"], "invalid -c 3 with -m 1: a fan call sends its tx blocks, not sequenced payloads"),
    (["-c", "3", "-w", "2", "-m", "2"], "invalid -c 3 with -m 2: a fan call sends its tx blocks, not sequenced payloads"),
    (["-c", "3", "-w", "1", "-H", "1"], "invalid -c 3 with -H 1: a host-link call sends its tx, not sequenced payloads"),
    (["-c", "3", "-w", "2", "-A", "1"], "invalid -c 3 with -A 1: a sequenced call cannot be armed ahead of the barrier"),
    (["-c", "3", "-w", "2", "-L", "64"], "invalid -c 3 with -L 64: sequenced calls are never traced by the latency recorder"),
    (["-c", "3", "-w", "2", "-i", "1000", "-b", "1048576"],
     "invalid -c 3 with -i 1000 and -b 1048576: more than 268435456 bytes of expected payloads to generate per run"),
    (["-c", "3", "-w", "2", "-i", "300", "-S", "1:1048576"],
     "invalid -c 3 with -i 300 and -b 1048576: more than 268435456 bytes of expected payloads to generate per run"),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_mpx_perf_refuses_c3_with(tmp_path, args, message):
    """a configuration error with its own line and exit status 255, before any
    GPU work (HIP_VISIBLE_DEVICES hides every device), and no log folder"""
    p = _perf(tmp_path, args)
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message + "\n" in p.stderr, p.stderr[-400:]
    assert p.stderr.count("invalid -c 3") == 1 and "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_c3_is_in_the_usage_text_and_valid_jobs_pass_validation(tmp_path):
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    assert "-c <checksum every payload 0|1|2|3 (2: seeded-pattern payloads, 3: a payload of its own per iteration)>" in p.stderr
    # the largest job that is not refused gets as far as the GPU (none visible here); -a 1 and -x 1 are allowed
    for extra in (["-i", "256", "-b", "1048576"], ["-a", "1", "-u", "1"], ["-x", "1"]):
        p = _perf(tmp_path, ["-c", "3", "-w", "2"] + extra)
        assert "invalid" not in p.stderr and p.returncode != 0, (extra, p.stderr[-400:])


def test_host_pattern_under_the_host_sanitizers(tmp_path):
    """tools/seq_host_check.cpp: a stand-alone program with its own main, built
    with -fsanitize=address,undefined, run once (CPU only; nothing is loaded
    into python)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "seq_host_check"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tools", "seq_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-1500:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert p.stdout == "seq_host_check: ok\n"
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr


def test_kernel_registers_in_the_build_output(tmp_path):
    """The new kernels in the compiler's resource report, compiled with the
    flags the Makefile builds the library with: exactly k_xfer_seq's five
    instantiations and k_xfer_seq_nbcheck; each without scratch or spilled
    VGPRs, within 128 VGPRs and at four waves per SIMD or more (pairs that
    share a GPU rely on four workgroups per CU), and with no more SGPRs than
    the widest k_xfer.  DESIGN.md §5 "Sequenced payloads" records the figures."""
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
    new = {k: v for k, v in usage.items() if "seq" in k and "k_seqbase" not in k}
    pair = {k: v for k, v in usage.items() if re.search(r"6k_xferILi[012]ELi[01]E", k)}
    assert sorted(new) == sorted(["_ZN3mpx10k_xfer_seqILi%dELi%dEEEvNS_8XferArgsE" % mg for mg in
                                  ((0, 0), (0, 1), (1, 0), (2, 0), (2, 1))] + ["_ZN3mpx18k_xfer_seq_nbcheckENS_8XferArgsE"])
    assert len(pair) == 5, sorted(pair)
    print(new)
    for k, v in new.items():
        assert v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4, (k, v)
        assert v["TotalSGPRs"] <= max(x["TotalSGPRs"] for x in pair.values()), (k, v)
    src = open(os.path.join(PKG, "csrc", "mpx_kernels.hip")).read()
    for kernel in ("k_xfer_seq(XferArgs a)", "k_xfer_seq_nbcheck(XferArgs a)"):
        assert "__global__ __launch_bounds__(kBlock, 4) void " + kernel in src, kernel
