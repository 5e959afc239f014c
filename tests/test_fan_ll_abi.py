"""MPX_FAN_LL's C-ABI and mpx_perf's -m 2 — everything that needs no GPU.  The
exchange itself runs in tests/test_gpu_fan_ll.py.
"""
import ctypes as C
import os
import re
import subprocess

import pytest

import mpx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERF = os.path.join(ROOT, "mpi-perf_amd", "bin", "mpx_perf")
OLD_M_LINE = "-m <1: every run is one fan exchange, each rank with all others at once (kernel engine)>\n"


def test_the_flag_its_cap_and_the_abi_version():
    txt = open(mpx.HEADER_PATH).read()
    assert re.search(r"^#define MPX_FAN_LL 8\b", txt, flags=re.M)
    assert re.search(r"^#define MPX_FAN_LL_MAX 4096\b", txt, flags=re.M)
    assert "#define MPX_ABI_VERSION 7\n" in txt and mpx.ABI_VERSION == 7 and mpx.lib().mpx_version() == 7
    assert mpx.XFER_FAN_LL == 8 and mpx.FAN_LL_MAX == 4096 and mpx.PROTO_FAN_LL == 10
    # a bit no pair flag uses
    assert mpx.XFER_FAN_LL & (mpx.XFER_STREAM | mpx.XFER_PULL | mpx.XFER_NOSTAGE) == 0
    assert "10 = lock-step LL fan exchange (MPX_FAN_LL)" in txt


def test_argument_checks_without_a_context():
    """the NULL checks come first, with the flag as without it"""
    L = mpx.lib()
    peers = (C.c_int * 1)(1)
    t = mpx.Timing()
    o = mpx.FanOpts(check=0, flags=mpx.XFER_FAN_LL, timeout_ms=0, nwg=0, expect_checksum=None)
    assert L.mpx_xfer_fan(None, 0, 1, peers, 1, None, None, 8, 16, C.byref(o), C.byref(t), None) == mpx.ERR_INVALID
    assert b"NULL" in L.mpx_last_error()


def perf(tmp_path, world, extra):
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc,runsc,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1")
    return subprocess.run([PERF, "-w", str(world), "-f", str(g1), "-n", "1", "-p", str(world // 2), "-l",
                           str(tmp_path / "logs"), *extra], capture_output=True, text=True, env=env, timeout=60)


REFUSALS = [
    (["-b", "4097"], 3, "invalid -m 2 with -b 4097: a lock-step LL fan block is at most 4096 bytes\n"),
    (["-S", "1024:8192"], 3, "invalid -m 2 with -b 8192: a lock-step LL fan block is at most 4096 bytes\n"),
    (["-a", "1"], 4, "invalid -m 2 with -a 1: a fan run already has every rank exchange with all others\n"),
    (["-A", "1"], 3, "invalid -m 2 with -A 1: a fan call cannot be armed ahead of the barrier\n"),
    (["-L", "64"], 3, "invalid -m 2 with -L 64: fan calls are never traced by the latency recorder\n"),
    (["-e", "sdma"], 3, "invalid -m 2 with -e sdma|rccl: the fan exchange runs on the kernel engine only\n"),
    (["-e", "rccl"], 3, "invalid -m 2 with -e sdma|rccl: the fan exchange runs on the kernel engine only\n"),
    (["-d", "1"], 3, "invalid -m 2 with -d 1: the .NET launcher lines describe pairs\n"),
    (["-b", "8"], 1, "invalid -m 2 with 1 rank: a fan run needs at least 2\n"),
    (["-b", str((1 << 31) - 1)], 3, "invalid -m 2 with -b 2147483647: 3 blocks of 2147483648 bytes exceed the largest buffer "
                                   "a rank can attach\n"),
]


@pytest.mark.parametrize("extra,world,message", REFUSALS)
def test_mpx_perf_refuses_m2_with(tmp_path, extra, world, message):
    """a configuration error with its exact message and exit status 255, before
    any GPU work: HIP_VISIBLE_DEVICES hides every device"""
    p = perf(tmp_path, world, ["-m", "2", *extra])
    assert p.returncode == 255, (p.returncode, p.stderr[-400:])
    assert message in p.stderr, p.stderr[-400:]
    assert "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()


def test_m1_messages_stay_and_m1_takes_any_block(tmp_path):
    p = perf(tmp_path, 4, ["-m", "1", "-a", "1"])
    assert p.returncode == 255
    assert "invalid -m 1 with -a 1: a fan run already has every rank exchange with all others\n" in p.stderr
    p = perf(tmp_path, 3, ["-m", "1", "-b", "4097"])
    assert "invalid -m" not in p.stderr, p.stderr[-400:]


def test_m2_at_the_cap_passes_validation(tmp_path):
    """-m 2 -b 4096 gets past every configuration check: what fails then is the
    hidden GPU, not an `invalid` message"""
    for extra in (["-b", "4096"], ["-b", "8"], ["-S", "8:4096"], ["-b", "4096", "-A", "0"]):
        p = perf(tmp_path, 3, ["-m", "2", *extra])
        assert "invalid" not in p.stderr, (extra, p.stderr[-400:])
        assert p.returncode != 0                       # no device to run on


def test_usage_text_holds_both_lines():
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 255
    at = p.stderr.index(OLD_M_LINE)
    assert at > p.stderr.index("MI355X extensions:")
    rest = p.stderr[at + len(OLD_M_LINE):]
    assert rest.lstrip().startswith("<2: the same as a lock-step exchange of LL granules, -b up to 4096 (MPX_FAN_LL)>"), rest
