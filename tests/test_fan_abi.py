"""The fan exchange's C-ABI (include/mpx.h mpx_xfer_fan), its width rule and
block layout, and mpx_perf's -m option — everything that needs no GPU.  The
exchange itself runs in tests/test_gpu_fan.py.

The width rule is held against the library's exported helper mpx_fan_width
(not against values a GPU run prints): tests/fan.py restates the rule in
Python, this file compares the two over the sizes, worlds and overrides the
GPU tests use and many more.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import mpx
from fan import fan_width, pair_nwg, round16
from payload import chunk_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
PERF = os.path.join(ROOT, "mpi-perf_amd", "bin", "mpx_perf")
HOST_LIB = os.path.join(ROOT, "mpi-perf_amd", "lib", "libmpx_host.so")
FAN_FUNCS = ["mpx_fan_width", "mpx_xfer_fan"]


def test_fan_symbols_declared_exported_and_bound():
    assert [s for s in mpx.header_symbols() if "fan" in s] == FAN_FUNCS
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for s in FAN_FUNCS:
        assert f" T {s}\n" in dyn, s
        assert s in mpx._SIGS, s
    # no ABI bump: callers detect the feature by symbol
    assert mpx.lib().mpx_version() == 7 and mpx.ABI_VERSION == 7
    assert mpx.PROTOCOLS[9] == "fan" and len(mpx.PROTOCOLS) == 10
    assert hasattr(mpx.Context, "fan")
    txt = open(mpx.HEADER_PATH).read()
    assert ("int mpx_xfer_fan(mpx_ctx *ctx, int my_rank, int npeers, const int *peers, int iters, void *tx, void *rx,\n"
            "                 int block_len, size_t stride, const mpx_fan_opts *opts, mpx_timing *t,\n") in txt


def test_fan_struct_layouts_match_the_header(tmp_path):
    """mpx_fan_opts and mpx_fan_link have the binding's size and field
    offsets: a C program built against include/mpx.h prints them"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    mirrors = {"mpx_fan_opts": mpx.FanOpts, "mpx_fan_link": mpx.FanLink}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "mpx.h"', "int main(void) {"]
    for cname, py in mirrors.items():
        src.append(f'    printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            src.append(f'    printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    src += ["    return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", INC, str(c), "-o", str(exe)], check=True, capture_output=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        name, field, val = line.split()
        got[(name, field)] = int(val)
    for cname, py in mirrors.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert C.sizeof(mpx.FanOpts) == 24 and C.sizeof(mpx.FanLink) == 40


def test_fan_argument_validation_without_gpu():
    L = mpx.lib()
    peers = (C.c_int * 1)(1)
    t = mpx.Timing()
    assert L.mpx_xfer_fan(None, 0, 1, peers, 1, None, None, 8, 16, None, C.byref(t), None) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()
    assert L.mpx_fan_width(1, 8, 1, 0) == -1 and L.mpx_fan_width(65, 8, 1, 0) == -1
    assert L.mpx_fan_width(4, -1, 1, 0) == -1 and L.mpx_fan_width(4, 8, 1, -1) == -1
    assert L.mpx_fan_width(4, 1 << 20, 1, 257) == -1          # wider than a link's flag words


SIZES = [0, 1, 15, 16, 17, 1023, 1024, 1025, 2049, 4097, 16384, 16385, 65555, 98305, 456131, 1 << 20, (1 << 20) + 1,
         4 << 20, (1 << 31) - 1]


def test_width_rule_python_and_library_agree(monkeypatch):
    monkeypatch.delenv("MPX_FAN_WG", raising=False)
    for nranks in (2, 3, 4, 5, 8, 9, 33, 64):
        for n in SIZES:
            for same in (True, False):
                assert mpx.fan_width(nranks, n, same) == fan_width(nranks, n, same), (nranks, n, same)
                for nwg in (1, 7, 96, 200, 256):
                    assert mpx.fan_width(nranks, n, same, nwg) == fan_width(nranks, n, same, nwg=nwg), (nranks, n, nwg)
    # the figures the documents and the GPU tests quote
    assert fan_width(8, 4 << 20) == 18 and 8 * 7 * 18 <= 1024          # a full node's ranks on one GPU stay resident
    assert fan_width(3, 65555) == 5 and fan_width(4, 65555) == 5 and fan_width(2, 456131) == 28
    assert fan_width(3, 98305, nwg=96) == 96 and chunk_shape(96, 98305)[0] == 96
    assert fan_width(2, 4 << 20) == 128 == pair_nwg(4 << 20)
    # the environment's override, below the call's own and above the default; narrowed like both
    monkeypatch.setenv("MPX_FAN_WG", "8")
    for n in SIZES:
        assert mpx.fan_width(8, n) == fan_width(8, n, env=8), n
        assert mpx.fan_width(8, n, True, 40) == fan_width(8, n, nwg=40, env=8), n
    assert mpx.fan_width(8, 4 << 20) == 8 and mpx.fan_width(8, 4097) == 5


def test_block_layout_python_and_host_library_agree():
    """mpx_perf -m 1's layout (block j at j * stride, stride = -b rounded up
    to 4096, world blocks per buffer, refused past 2^31 - 1) against its
    Python restatement, and the stride rule the GPU tests use"""
    H = C.CDLL(HOST_LIB)
    H.mpxh_fan_stride.restype = C.c_size_t
    H.mpxh_fan_stride.argtypes = [C.c_int]
    H.mpxh_fan_bytes.restype = C.c_size_t
    H.mpxh_fan_bytes.argtypes = [C.c_int, C.c_int]
    H.mpxh_fan_peers.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    for n in SIZES:
        stride = (n + 4095) // 4096 * 4096
        assert H.mpxh_fan_stride(n) == stride and stride % 16 == 0 and stride >= n
        assert round16(n) % 16 == 0 and n <= round16(n) < n + 16
        for world in (2, 3, 8, 64):
            total = world * stride
            assert H.mpxh_fan_bytes(world, n) == (total if total <= (1 << 31) - 1 else 0), (world, n)
            # block j of a rank's buffer, and the last block's end, lie inside it
            assert all(j * stride + n <= total for j in range(world))
    for world in (2, 3, 8):
        for r in range(world):
            buf = (C.c_int * 64)()
            assert H.mpxh_fan_peers(world, r, buf) == world - 1
            assert list(buf[:world - 1]) == [q for q in range(world) if q != r]


REFUSALS = [
    (["-a", "1"], 4, "invalid -m 1 with -a 1"),
    (["-A", "1"], 3, "invalid -m 1 with -A 1"),
    (["-L", "64"], 3, "invalid -m 1 with -L 64"),
    (["-e", "sdma"], 3, "invalid -m 1 with -e sdma|rccl"),
    (["-e", "rccl"], 3, "invalid -m 1 with -e sdma|rccl"),
    (["-d", "1"], 3, "invalid -m 1 with -d 1"),
    (["-b", str((1 << 31) - 1)], 3, "invalid -m 1 with -b 2147483647"),
]


@pytest.mark.parametrize("extra,world,message", REFUSALS)
def test_mpx_perf_refuses_m_with(tmp_path, extra, world, message):
    """a configuration error with its own message and exit status 255, before
    any GPU work: HIP_VISIBLE_DEVICES hides every device"""
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc,runsc,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([PERF, "-w", str(world), "-f", str(g1), "-n", "1", "-p", str(world // 2), "-l",
                        str(tmp_path / "logs"), "-m", "1", *extra], capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message in p.stderr, p.stderr[-400:]
    assert "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_m_is_parsed_and_in_the_usage_text(tmp_path):
    """-m alone passes validation (an explicit -A 0 too); the usage text names
    it in the extension part, after the reference's own text"""
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 255
    ext = p.stderr.index("MI355X extensions:")
    assert p.stderr.index("-m <1: every run is one fan exchange") > ext > p.stderr.index("-x <use non-blocking MPI calls>")


def test_fan_host_arithmetic_under_the_host_sanitizers(tmp_path):
    """tools/asan_fan.sh: the link table's map and widths and mpx_perf's fan
    arithmetic in a stand-alone program built with -fsanitize=address,undefined
    (CPU only; nothing is loaded into python)"""
    if shutil.which("g++") is None or shutil.which("gcc") is None:
        pytest.skip("no C/C++ compiler")
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_fan.sh"), str(tmp_path)], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-1500:])
    assert "fan_host_check: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
