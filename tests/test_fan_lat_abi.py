"""The link recorder's C-ABI (include/mpx_fan_lat.h, part of include/mpx.h: mpx_fan_lat_*) and mpx_perf's -P
option — everything that needs no GPU.  The recorder itself runs in
tests/test_gpu_fan_lat.py.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import mpx
from test_fan_ll_abi import OLD_M_LINE, PERF, perf

FAN_LAT_FUNCS = ["mpx_fan_lat_disable", "mpx_fan_lat_enable", "mpx_fan_lat_get", "mpx_fan_lat_raw", "mpx_fan_lat_reset"]
M2_LINE = "<2: the same as a lock-step exchange of LL granules, -b up to 4096 (MPX_FAN_LL)>\n"


DECL_C = r"""
#include "mpx.h"   /* alone: it brings the link recorder's declarations with it */
int (*p_enable)(mpx_ctx *, int, int) = mpx_fan_lat_enable;
int (*p_disable)(mpx_ctx *, int) = mpx_fan_lat_disable;
int (*p_reset)(mpx_ctx *, int) = mpx_fan_lat_reset;
int (*p_get)(mpx_ctx *, int, int, mpx_lat *) = mpx_fan_lat_get;
int (*p_raw)(mpx_ctx *, int, int, uint64_t *, int, int *) = mpx_fan_lat_raw;
_Static_assert(MPX_FAN_LAT_RAW_MAX == 65536, "MPX_FAN_LAT_RAW_MAX");
_Static_assert(MPX_ABI_VERSION == 7, "MPX_ABI_VERSION");
int main(void) { return !(p_enable && p_disable && p_reset && p_get && p_raw); }
"""


def test_fan_lat_functions_declared_and_exported(tmp_path):
    """The five functions are declared by including mpx.h alone, with these
    prototypes (a C translation unit that takes their addresses), and exported.
    Their declarations stand in include/mpx_fan_lat.h, which mpx.h includes:
    mpx.h's own text keeps the two fan functions it had."""
    inc = os.path.dirname(mpx.HEADER_PATH)
    sub = os.path.join(inc, "mpx_fan_lat.h")
    assert sorted(mpx.header_symbols(sub)) == FAN_LAT_FUNCS
    txt = open(mpx.HEADER_PATH).read()
    assert re.search(r'^#include "mpx_fan_lat\.h"$', txt, flags=re.M)
    assert re.search(r"^#define MPX_FAN_LAT_RAW_MAX \(1 << 16\)", open(sub).read(), flags=re.M)
    assert mpx.FAN_LAT_RAW_MAX == 65536
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for f in FAN_LAT_FUNCS:
        assert f" T {f}\n" in dyn, f
        assert f in mpx._SIGS, f
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "decl.c"
    src.write_text(DECL_C)
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "decl.o")],
                   check=True, capture_output=True)
    L = mpx.lib()
    assert "#define MPX_ABI_VERSION 7\n" in txt and mpx.ABI_VERSION == 7 and L.mpx_version() == 7
    # the rank recorder's names and limit stay what they were
    assert mpx.LAT_RAW_MAX == 1 << 22 and re.search(r"^#define MPX_LAT_RAW_MAX \(1 << 22\)", txt, flags=re.M)


def test_fan_lat_null_context():
    L = mpx.lib()
    lat, n = mpx.Lat(), C.c_int(-1)
    buf = (C.c_uint64 * 4)()
    assert L.mpx_fan_lat_enable(None, 0, 16) == mpx.ERR_INVALID
    assert L.mpx_fan_lat_disable(None, 0) == mpx.ERR_INVALID
    assert L.mpx_fan_lat_reset(None, 0) == mpx.ERR_INVALID
    assert L.mpx_fan_lat_get(None, 0, 1, C.byref(lat)) == mpx.ERR_INVALID
    assert L.mpx_fan_lat_raw(None, 0, 1, buf, 4, C.byref(n)) == mpx.ERR_INVALID
    assert L.mpx_last_error()


def test_P_passes_validation_with_m2(tmp_path):
    """what fails then is the hidden GPU, not a configuration message"""
    for extra in (["-P", "64", "-b", "8"], ["-P", "0", "-b", "8"], ["-P", "65536", "-b", "4096"]):
        p = perf(tmp_path, 3, ["-m", "2", *extra])
        assert "invalid" not in p.stderr and "bad value" not in p.stderr, (extra, p.stderr[-400:])
        assert p.returncode != 0                       # no device to run on


def test_P_without_m2_is_refused(tmp_path):
    for world, extra in ((2, ["-P", "64"]), (3, ["-m", "1", "-P", "64"])):
        p = perf(tmp_path, world, extra)
        assert p.returncode == 255, (extra, p.returncode, p.stderr[-400:])
        assert "invalid -P 64 without -m 2:" in p.stderr, (extra, p.stderr[-400:])
        assert "mpx call failed" not in p.stderr
        assert not (tmp_path / "logs").exists()


def test_P_bad_values(tmp_path):
    for bad in ("-1", "x", "65537"):
        p = perf(tmp_path, 3, ["-m", "2", "-P", bad])
        assert p.returncode == 255, (bad, p.returncode)
        assert "bad value" in p.stderr and "invalid" not in p.stderr, (bad, p.stderr[-400:])
        assert not (tmp_path / "logs").exists()


def test_m2_with_L_is_still_refused_with_its_old_text(tmp_path):
    for extra in (["-L", "64"], ["-L", "64", "-P", "64"]):
        p = perf(tmp_path, 3, ["-m", "2", *extra])
        assert p.returncode == 255
        assert "invalid -m 2 with -L 64: fan calls are never traced by the latency recorder\n" in p.stderr
    p = perf(tmp_path, 3, ["-m", "1", "-L", "64"])
    assert "invalid -m 1 with -L 64: fan calls are never traced by the latency recorder\n" in p.stderr


def test_usage_text_names_P_below_the_m_lines():
    p = subprocess.run([PERF, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 255
    at = p.stderr.index(OLD_M_LINE)
    rest = p.stderr[at + len(OLD_M_LINE):]
    assert rest.lstrip().startswith(M2_LINE.strip()), rest
    after = rest[rest.index(M2_LINE) + len(M2_LINE):]
    assert after.lstrip().startswith("-P <raw-cap: with -m 2, record every link's per-iteration exchange latency"), after
