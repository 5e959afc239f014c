"""The C-ABI of the sequenced fan payloads (include/mpx_fan_seq.h), mpx_perf's
-Q, the helpers of the GPU tests (tests/fan_seq.py) and the kernels' resource
report — everything that needs no GPU.  The calls themselves run in
tests/test_gpu_fan_seq.py.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import fan_seq as S
import mpx
import payload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
PKG = os.path.join(ROOT, "mpi-perf_amd")
PERF = os.path.join(PKG, "bin", "mpx_perf")


def _header_functions(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(mpx_[a-z_0-9]+)\s*\(", txt, flags=re.M)))


# ---- header ---------------------------------------------------------------------------
def test_symbol_declared_exported_and_bound():
    assert _header_functions(os.path.join(INC, "mpx_fan_seq.h")) == ["mpx_xfer_fan_seq"]
    # part of mpx.h, inside its extern "C" block, after mpx_seq.h; declared nowhere else
    txt = open(mpx.HEADER_PATH).read()
    assert txt.index('#include "mpx_seq.h"') < txt.index('#include "mpx_fan_seq.h"') < txt.index("#ifdef __cplusplus\n}")
    for other in ("mpx.h", "mpx_seq.h", "mpx_fan_lat.h"):
        assert "mpx_xfer_fan_seq" not in _header_functions(os.path.join(INC, other)), other
    hdr = open(os.path.join(INC, "mpx_fan_seq.h")).read()
    assert "#ifndef MPX_H\n#error" in hdr
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    assert " T mpx_xfer_fan_seq\n" in dyn and "mpx_xfer_fan_seq" in mpx._SIGS
    # no ABI bump: callers detect the feature by symbol
    assert mpx.lib().mpx_version() == 7 and mpx.ABI_VERSION == 7 and "#define MPX_ABI_VERSION 7" in txt
    assert hasattr(mpx.Context, "xfer_fan_seq")
    sig, fan = mpx._SIGS["mpx_xfer_fan_seq"], mpx._SIGS["mpx_xfer_fan"]
    assert sig[0] == fan[0] and sig[1][:9] == fan[1][:9] and sig[1][10:] == fan[1][10:]
    assert sig[1][9] == C.POINTER(mpx.FanSeqOpts)


def test_struct_layout_matches_the_header(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "mpx.h"', "int main() {",
           '    printf("size %zu\\n", sizeof(mpx_fan_seq_opts));']
    for f, _ in mpx.FanSeqOpts._fields_:
        src.append(f'    printf("{f} %zu\\n", offsetof(mpx_fan_seq_opts, {f}));')
    src += ["    return 0;", "}"]
    c = tmp_path / "layout.cpp"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++17", "-I", INC, str(c), "-o", str(exe)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(mpx.FanSeqOpts) == 32
    for f, _ in mpx.FanSeqOpts._fields_:
        assert int(got[f]) == getattr(mpx.FanSeqOpts, f).offset, f
    assert [f for f, _ in mpx.FanSeqOpts._fields_] == ["seed", "check", "flags", "timeout_ms", "nwg", "expect"]


def test_null_arguments_without_a_gpu():
    L = mpx.lib()
    t, o = mpx.Timing(), mpx.FanSeqOpts()
    peers = (C.c_int * 1)(1)
    dummy = C.create_string_buffer(64)
    a = (0, 1, peers, 1, None, None, 8, 16)
    assert L.mpx_xfer_fan_seq(None, *a, C.byref(o), C.byref(t), None) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()
    # NULL peers / opts / timing, with a pointer in ctx's place: refused before ctx is looked at
    assert L.mpx_xfer_fan_seq(dummy, 0, 1, None, 1, None, None, 8, 16, C.byref(o), C.byref(t), None) == mpx.ERR_INVALID
    assert L.mpx_xfer_fan_seq(dummy, *a, None, C.byref(t), None) == mpx.ERR_INVALID
    assert L.mpx_xfer_fan_seq(dummy, *a, C.byref(o), None, None) == mpx.ERR_INVALID


# ---- mpx_perf -Q ----------------------------------------------------------------------
def _perf(tmp_path, args):
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([PERF, "-f", str(g1), "-n", "1", "-p", "1", "-l", str(tmp_path / "logs"), *args],
                          capture_output=True, text=True, env=env, timeout=60)


C3_M = "invalid -c 3 with -m %d: a fan call sends its tx blocks, not sequenced payloads"
REFUSALS = [
    (["-Q", "2", "-m", "1", "-w", "2"], "invalid -Q: its value is 0 or 1"),
    (["-Q", "x", "-m", "1", "-w", "2"], "invalid -Q: its value is 0 or 1"),
    (["-Q", "-1", "-m", "2", "-w", "2"], "invalid -Q: its value is 0 or 1"),
    (["-Q", "1", "-w", "2"], "invalid -Q 1 without -m: sequenced fan payloads are a fan run's (-c 3 is the pair loops')"),
    (["-Q", "1", "-w", "2", "-c", "3"],
     "invalid -Q 1 without -m: sequenced fan payloads are a fan run's (-c 3 is the pair loops')"),
    (["-Q", "1", "-m", "1", "-w", "2", "-c", "2"], "invalid -Q 1 with -c 2: a sequenced fan call does not send tx"),
    (["-Q", "1", "-m", "2", "-w", "2", "-c", "2"], "invalid -Q 1 with -c 2: a sequenced fan call does not send tx"),
    (["-Q", "1", "-m", "2", "-w", "2", "-P", "64"],
     "invalid -Q 1 with -P 64: sequenced fan calls are never traced by the link recorder"),
    (["-Q", "1", "-m", "1", "-w", "3", "-c", "1", "-i", "1000", "-b", "1048576"],
     "invalid -Q 1 -c 1 with 2 peers, -i 1000 and -b 1048576: more than 268435456 bytes of expected payloads to generate per run"),
    (["-Q", "1", "-m", "1", "-w", "2", "-c", "1", "-i", "300", "-S", "1:1048576"],
     "invalid -Q 1 -c 1 with 1 peers, -i 300 and -b 1048576: more than 268435456 bytes of expected payloads to generate per run"),
    # -c 3 with -m keeps its own refusal and text, whatever -Q says
    (["-Q", "1", "-m", "1", "-w", "2", "-c", "3"], C3_M % 1),
    (["-Q", "1", "-m", "2", "-w", "2", "-c", "3"], C3_M % 2),
    (["-Q", "7", "-m", "1", "-w", "2", "-c", "3"], C3_M % 1),
]


@pytest.mark.parametrize("args,message", REFUSALS)
def test_mpx_perf_refuses(tmp_path, args, message):
    """a configuration error with a line of its own and exit status 255, before
    any GPU work (HIP_VISIBLE_DEVICES hides every device), and no log folder"""
    p = _perf(tmp_path, args)
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message + "\n" in p.stderr, p.stderr[-400:]
    assert p.stderr.count("invalid -") == 1 and p.stderr.count(message) == 1 and "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_Q_is_in_the_usage_text_and_valid_jobs_pass_validation(tmp_path):
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    line = "-Q <1: with -m 1|2, every run is one sequenced fan call: a payload per (src, dst, iteration); -c 0|1>"
    assert line in p.stderr
    assert p.stderr.index("-P <raw-cap: with -m 2") < p.stderr.index(line)
    # jobs that are not refused get as far as the GPU (none visible here); the largest -c 1 job, -c 0 beyond it, -Q 0
    for extra in (["-Q", "1", "-m", "1", "-c", "1", "-i", "256", "-b", "1048576"], ["-Q", "1", "-m", "2", "-c", "0", "-b", "2045"],
                  ["-Q", "1", "-m", "1", "-i", "1000", "-b", "1048576"], ["-Q", "0", "-m", "1", "-c", "2"], ["-Q", "0"]):
        p = _perf(tmp_path, ["-w", "2"] + extra)
        assert "invalid" not in p.stderr and p.returncode != 0, (extra, p.stderr[-400:])


# ---- the GPU tests' helper: only the right rx passes ------------------------------------
def _fake(n=2045, nranks=4, r=1, iters=5):
    stride = ((n + 15) & ~15) + 16
    cap = nranks * stride + payload.GUARD
    peers = [3, 0, 2]
    return n, stride, cap, r, peers, iters


def test_expected_rx_builder_accepts_only_the_right_bytes():
    n, stride, cap, r, peers, iters = _fake()
    right = S.expected_rx(cap, stride, n, r, peers, iters - 1)
    S.check_rx(right, cap, stride, n, r, peers, iters - 1, "right")
    assert right[r * stride:(r + 1) * stride] == bytes([0xEE]) * stride and right[-payload.GUARD:] == bytes([0xEE]) * payload.GUARD
    for p in peers:
        assert right[p * stride:p * stride + n] == S.sent(S.SEED, p, r, iters - 1, n) and right[p * stride + n] == 0xEE

    def fails(img, where):
        with pytest.raises(AssertionError) as ei:
            S.check_rx(bytes(img), cap, stride, n, r, peers, iters - 1, "fake")
        assert where in str(ei.value), str(ei.value)

    lo = 3 * stride
    named = f"block of peer 3, iteration {iters - 1} [{lo}, {lo + n})"
    img = bytearray(right)                      # the block of the iteration before the last
    img[lo:lo + n] = S.sent(S.SEED, 3, r, iters - 2, n)
    fails(img, named)
    img = bytearray(right)                      # the key of (d, s) in (s, d)'s place
    img[lo:lo + n] = S.sent(S.SEED, r, 3, iters - 1, n)
    fails(img, named)
    img = bytearray(right)                      # another link's key
    img[lo:lo + n] = S.sent(S.SEED, 0, r, iters - 1, n)
    fails(img, named)
    img = bytearray(right)                      # another seed
    img[lo:lo + n] = S.sent(S.SEED + 1, 3, r, iters - 1, n)
    fails(img, named)
    img = bytearray(right)                      # one byte of a gap
    img[2 * stride + n + 3] = 0
    fails(img, f"gap after block 2 [{2 * stride + n}, {3 * stride})")
    img = bytearray(right)                      # the rank's own block
    img[r * stride + 5] = 1
    fails(img, f"untouched block {r} [{r * stride}, {r * stride + n})")
    img = bytearray(right)                      # the guard behind the last block
    img[cap - 1] = 0
    fails(img, f"guard [{4 * stride}, {cap})")
    # nothing moved: everything is 0xEE, and a moved block fails
    S.check_rx(bytes([0xEE]) * cap, cap, stride, n, r, peers, -1, "nothing moved")
    fails(bytes([0xEE]) * cap, f"block of peer 0, iteration {iters - 1} [0, {n})")


def test_expectations_layout_is_link_major_from_host_bytes():
    import oracle_py as O
    n, _, _, r, peers, iters = _fake()
    e = S.expectations(r, peers, n, iters)
    assert len(e) == len(set(e)) == len(peers) * iters
    for k, p in enumerate(peers):
        for i in range(iters):
            assert e[k * iters + i] == O.checksum(O.fill(n, mpx.FILL_SPLITMIX, mpx.pattern_key(S.SEED, p, r, i)))
            assert e[k * iters + i] == mpx.seq_expect(S.SEED, p, r, i, n)


# ---- host check under the sanitizers --------------------------------------------------
def test_fan_seq_arithmetic_under_the_host_sanitizers(tmp_path):
    """tools/fan_seq_host_check.cpp: a stand-alone program with its own main,
    built with -fsanitize=address,undefined, run once (CPU only; nothing is
    loaded into python)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "fan_seq_host_check"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tools", "fan_seq_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-1500:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert p.stdout == "fan_seq_host_check: ok\n"
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr
    src = open(os.path.join(ROOT, "tools", "fan_seq_host_check.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["mpx_seq.h"]


# ---- resource report --------------------------------------------------------------------
# The ordinary fan kernels' figures in the report of the commit before the
# sequenced fan payloads (979f766), compiled with the Makefile's flags:
# (TotalSGPRs, VGPRs, Occupancy, SGPRs Spill), each with no AGPRs, no scratch,
# no spilled VGPRs and 40 bytes of LDS.  Written from that report, not from
# this tree's.
FAN = "_ZN3mpx10k_xfer_fanILb%dELb%dEEEvNS_7FanArgsE"
FAN_LL = "_ZN3mpx13k_xfer_fan_llILb%dELb%dELb%dEEEvNS_9FanLLArgsE"
PARENT = {
    FAN % (0, 0): (67, 48, 8, 0),
    FAN % (1, 0): (78, 73, 6, 38),
    FAN_LL % (0, 0, 0): (78, 37, 8, 25),
    FAN_LL % (0, 1, 0): (78, 50, 8, 29),
    FAN_LL % (1, 0, 0): (78, 45, 8, 38),
    FAN_LL % (1, 1, 0): (78, 58, 8, 41),
}
NEW = [FAN % (0, 1), FAN % (1, 1), FAN_LL % (0, 0, 1), FAN_LL % (1, 0, 1)]


def test_kernel_registers_in_the_build_output(tmp_path):
    """mpx_kernels.hip compiled with the flags the Makefile builds the library
    with: k_xfer_fan and k_xfer_fan_ll have exactly the expected
    instantiations (no traced sequenced one); the ordinary ones report the
    parent's figures; the new ones need no scratch, no spilled VGPRs and no
    AGPRs, and stay within 128 VGPRs at four waves per SIMD or more (ranks that
    share a GPU rely on four workgroups per CU); no kernel but the six pair
    kernels and k_seqbase has "seq" in its name.  DESIGN.md §5 "Sequenced fan
    payloads" records the figures."""
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
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs|SGPRs Spill|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split(" [")[0]] = int(m.group(2))
    fan = {k: v for k, v in usage.items() if "k_xfer_fan" in k}
    assert sorted(fan) == sorted(list(PARENT) + NEW)
    for k, (sgpr, vgpr, occ, spill) in PARENT.items():
        v = fan[k]
        assert (v["TotalSGPRs"], v["VGPRs"], v["Occupancy"], v["SGPRs Spill"]) == (sgpr, vgpr, occ, spill), (k, v)
        assert v["AGPRs"] == 0 and v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["LDS Size"] == 40, (k, v)
    print({k: fan[k] for k in NEW})
    for k in NEW:
        v = fan[k]
        assert v["ScratchSize"] == 0 and v["AGPRs"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128 and v["Occupancy"] >= 4 and v["TotalSGPRs"] <= 80, (k, v)
    seq = sorted(k for k in usage if "seq" in k)
    assert len(seq) == 7 and sum("k_seqbase" in k for k in seq) == 1, seq
    assert all(re.search(r"k_xfer_seq(ILi[012]ELi[01]E|_nbcheck)", k) or "k_seqbase" in k for k in seq), seq
    src = open(os.path.join(PKG, "csrc", "mpx_kernels.hip")).read()
    for kernel in ("k_xfer_fan(FanArgs f)", "k_xfer_fan_ll(FanLLArgs q)"):
        assert "__global__ __launch_bounds__(kBlock, 4) __attribute__((amdgpu_num_sgpr(80))) void " + kernel in src, kernel
