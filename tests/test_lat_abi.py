"""The per-iteration latency recorder's C-ABI (include/mpx.h mpx_lat_*), its
bucket rule and quantile, and mpx_perf's -L option — everything that needs no
GPU.  The recorder itself runs in tests/test_gpu_lat.py.
"""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import mpx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
PERF = os.path.join(ROOT, "mpi-perf_amd", "bin", "mpx_perf")
HOST_DIR = os.path.join(ROOT, "mpi-perf_amd", "host")
LIB_DIR = os.path.join(ROOT, "mpi-perf_amd", "lib")
LAT_FUNCS = ["mpx_lat_disable", "mpx_lat_enable", "mpx_lat_get", "mpx_lat_raw", "mpx_lat_reset"]


def cc():
    c = shutil.which("gcc") or shutil.which("cc")
    if c is None:
        pytest.skip("no C compiler")
    return c


def build_and_run(tmp_path, name, text, stdin="", extra=()):
    src = tmp_path / f"{name}.c"
    src.write_text(text)
    exe = tmp_path / name
    subprocess.run([cc(), "-std=c11", "-O1", "-I", INC, str(src), "-o", str(exe), *extra], check=True,
                   capture_output=True)
    return subprocess.run([str(exe)], input=stdin, check=True, capture_output=True, text=True).stdout


def test_lat_functions_declared_and_exported():
    assert [s for s in mpx.header_symbols() if s.startswith("mpx_lat_")] == LAT_FUNCS
    dyn = subprocess.run(["nm", "-D", "--defined-only", mpx.LIB_PATH], capture_output=True, text=True).stdout
    for s in LAT_FUNCS:
        assert f" T {s}\n" in dyn, s
    # no ABI bump: callers detect the feature by symbol
    assert mpx.lib().mpx_version() == 7
    txt = open(mpx.HEADER_PATH).read()
    assert f"#define MPX_LAT_BUCKETS {mpx.LAT_BUCKETS}" in txt and mpx.LAT_BUCKETS == 464
    assert "#define MPX_LAT_RAW_MAX (1 << 22)" in txt and mpx.LAT_RAW_MAX == 1 << 22


def test_lat_struct_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in mpx.Lat._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "mpx.h"', "int main(void) {",
           '    printf("size %zu\\n", sizeof(mpx_lat));']
    src += [f'    printf("{f} %zu\\n", offsetof(mpx_lat, {f}));' for f in fields]
    src += ["    return 0;", "}"]
    got = dict(line.split() for line in build_and_run(tmp_path, "layout", "\n".join(src) + "\n").splitlines())
    assert int(got["size"]) == C.sizeof(mpx.Lat)
    for f in fields:
        assert int(got[f]) == getattr(mpx.Lat, f).offset, f
    assert mpx.Lat.hist.size == 4 * 464


def bucket_inputs():
    v = [0, 1, 31, 32, 33, 63, 64]
    for k in range(33):
        v += [x for x in ((1 << k) - 1, 1 << k, (1 << k) + 1) if x >= 0]
    v += [(1 << 32) - 1, 1 << 32, 1 << 63]
    rnd = random.Random(20240607)
    # every magnitude, not only the top bits: a random width, then a random value of that width
    v += [rnd.getrandbits(rnd.randint(1, 64)) for _ in range(10000)]
    return v


BUCKET_C = r"""
#include <inttypes.h>
#include <stdio.h>
#include "mpx.h"
int main(void) {
    uint64_t v;
    while (scanf("%" SCNu64, &v) == 1) {
        const int b = mpx_lat_bucket(v);
        printf("%d %" PRIu64 " %" PRIu64 "\n", b, mpx_lat_bucket_floor(b), mpx_lat_bucket_floor(b + 1));
    }
    return 0;
}
"""


def test_bucket_rule_c_and_python_agree(tmp_path):
    vals = bucket_inputs()
    out = build_and_run(tmp_path, "bucket", BUCKET_C, stdin="".join(f"{v}\n" for v in vals)).splitlines()
    assert len(out) == len(vals)
    got = {}
    for v, line in zip(vals, out):
        b, lo, hi = (int(x) for x in line.split())
        assert b == mpx.lat_bucket(v), v
        assert lo == mpx.lat_bucket_floor(b) and hi == mpx.lat_bucket_floor(b + 1), v
        assert 0 <= b < 464
        if v < 1 << 32:
            assert lo <= v < hi, (v, b, lo, hi)     # the bucket holds its value
            assert v < 32 and lo == v or (v - lo) * 16 <= lo  # exact below 32, <= 1/16 above
        else:
            assert b == 463
        got[v] = b
    # monotone over the inputs
    order = sorted(got)
    assert all(got[a] <= got[b] for a, b in zip(order, order[1:]))
    # the ends of the table
    assert mpx.lat_bucket(31) == 31 and mpx.lat_bucket(32) == 32 and mpx.lat_bucket(63) == 47
    assert mpx.lat_bucket(64) == 48 and mpx.lat_bucket((1 << 32) - 1) == 463 and mpx.lat_bucket(1 << 63) == 463
    assert mpx.lat_bucket_floor(32) == 32 and mpx.lat_bucket_floor(463) == 31 << 27
    assert mpx.lat_bucket_floor(464) == 1 << 32


QUANTILE_C = r"""
#include <inttypes.h>
#include <stdio.h>
#include <string.h>
#include "mpx.h"
int main(void) {
    static mpx_lat l;
    int nb;
    while (scanf("%d", &nb) == 1) {
        double q;
        memset(&l, 0, sizeof l);
        for (int k = 0; k < nb; ++k) {
            int b;
            uint32_t c;
            if (scanf("%d %" SCNu32, &b, &c) != 2) return 1;
            l.hist[b] = c;
            l.count += c;
        }
        if (scanf("%" SCNu64 " %" SCNu64 " %lf", &l.min_ticks, &l.max_ticks, &q) != 3) return 1;
        printf("%" PRIu64 "\n", mpx_lat_quantile(&l, q));
    }
    return 0;
}
"""

# (histogram {bucket: count}, min, max, q) -> ticks, worked by hand from the
# rule: the floor of the first bucket whose cumulative count reaches
# ceil(q * count), clamped to [min, max]
QUANTILE_CASES = [
    ({20: 7}, 20, 20, 0.0, 20), ({20: 7}, 20, 20, 0.5, 20), ({20: 7}, 20, 20, 1.0, 20),
    # one log-linear bucket [104, 108): its floor, clamped up to the minimum seen
    ({58: 5}, 105, 107, 0.5, 105), ({58: 5}, 105, 107, 1.0, 105), ({58: 5}, 104, 107, 0.0, 104),
    # two buckets, 3 + 1: ceil(0.5 * 4) = 2 -> the first, ceil(0.76 * 4) = 4 -> the second
    ({10: 3, 200: 1}, 10, 40000, 0.5, 10), ({10: 3, 200: 1}, 10, 40000, 0.75, 10),
    # bucket 200 = [49152, 51200): above max_ticks = 40000 it clamps down
    ({10: 3, 200: 1}, 10, 40000, 0.76, 40000), ({10: 3, 200: 1}, 10, 40000, 1.0, 40000),
    ({10: 3, 200: 1}, 10, 50000, 1.0, 49152), ({10: 3, 200: 1}, 10, 50000, 0.0, 10),
    # the clamp bucket: its floor is 31 << 27; max_ticks below it clamps down
    ({463: 2}, 1 << 32, 1 << 33, 0.5, 1 << 32), ({5: 1, 463: 1}, 5, 31 << 27, 1.0, 31 << 27),
    ({}, 0, 0, 0.5, 0),
]


def test_quantile_on_hand_made_histograms(tmp_path):
    assert mpx.lat_bucket_floor(200) == 49152 and mpx.lat_bucket_floor(58) == 104   # the cases' own arithmetic
    text = ""
    for hist, mn, mx, q, _ in QUANTILE_CASES:
        text += f"{len(hist)} " + " ".join(f"{b} {c}" for b, c in hist.items()) + f" {mn} {mx} {q!r}\n"
    out = [int(x) for x in build_and_run(tmp_path, "quantile", QUANTILE_C, stdin=text).split()]
    assert len(out) == len(QUANTILE_CASES)
    for (hist, mn, mx, q, want), got in zip(QUANTILE_CASES, out):
        assert got == want, (hist, mn, mx, q)
        h = [0] * 464
        for b, c in hist.items():
            h[b] = c
        py = mpx.lat_quantile({"count": sum(h), "hist": h, "min_ticks": mn, "max_ticks": mx}, q)
        assert py == want, (hist, mn, mx, q)


def test_lat_argument_validation_without_gpu():
    L = mpx.lib()
    lat, n = mpx.Lat(), C.c_int(-1)
    buf = (C.c_uint64 * 4)()
    assert L.mpx_lat_enable(None, 0, 16) == mpx.ERR_INVALID
    assert L.mpx_lat_disable(None, 0) == mpx.ERR_INVALID
    assert L.mpx_lat_reset(None, 0) == mpx.ERR_INVALID
    assert L.mpx_lat_get(None, 0, C.byref(lat)) == mpx.ERR_INVALID
    assert L.mpx_lat_raw(None, 0, buf, 4, C.byref(n)) == mpx.ERR_INVALID
    assert L.mpx_last_error()


PARSE_C = r"""
#include <stdio.h>
#include "mpx_host.h"
int main(int argc, char **argv) {
    mpxh_options o;
    mpxh_defaults(&o);
    const int dflt = o.lat_cap;
    const int st = mpxh_parse_args(&o, argc, argv);
    printf("%d %d %d %d\n", dflt, st, o.lat_cap, mpxh_validate(&o, 2, stderr));
    return 0;
}
"""


def test_parse_args_accepts_L(tmp_path):
    src = tmp_path / "parse.c"
    src.write_text(PARSE_C)
    exe = tmp_path / "parse"
    subprocess.run([cc(), "-std=c11", "-I", HOST_DIR, str(src), "-o", str(exe), "-L", LIB_DIR, "-lmpx_host",
                    f"-Wl,-rpath,{LIB_DIR}"], check=True, capture_output=True)
    base = ["-f", "g1", "-n", "1", "-p", "1"]

    def parse(*args):
        p = subprocess.run([str(exe), *base, *args], check=True, capture_output=True, text=True)
        return [int(x) for x in p.stdout.split()], p.stderr

    assert parse()[0] == [-1, 0, -1, 0]                       # unset: off
    assert parse("-L", "64")[0] == [-1, 0, 64, 0]
    assert parse("-L", "0")[0] == [-1, 0, 0, 0]
    assert parse("-L", "64", "-u", "1")[0] == [-1, 0, 64, 0]
    for bad in ("-1", "x", "12x", str((1 << 22) + 1)):
        assert parse("-L", bad)[0][1] == 2, bad                # MPXH_PARSE_BAD_VALUE
    got, err = parse("-L", "64", "-x", "1")
    assert got == [-1, 0, 64, 1] and "-L" in err and "-x 1" in err
    got, err = parse("-L", "64", "-e", "rccl")
    assert got == [-1, 0, 64, 1] and "-L" in err


@pytest.mark.parametrize("extra", [["-x", "1"], ["-e", "sdma"], ["-e", "rccl"]])
def test_mpx_perf_refuses_L_with_nonblocking_or_another_engine(tmp_path, extra):
    """a configuration error, reported before any GPU work: HIP_VISIBLE_DEVICES
    hides every device, and the message is the validator's, not a HIP error"""
    g1 = tmp_path / "group1"
    g1.write_text("vm\n")
    env = dict(os.environ, MPX_PROCESSOR_NAMES="vm,runsc", MPX_HOSTNAME="localhost", HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([PERF, "-w", "2", "-f", str(g1), "-n", "1", "-p", "1", "-l", str(tmp_path / "logs"),
                        "-L", "64", *extra], capture_output=True, text=True, env=env, timeout=60)
    assert p.returncode != 0
    assert "invalid -L 64" in p.stderr, p.stderr[-400:]
    assert "mpx call failed" not in p.stderr
    assert not (tmp_path / "logs").exists()
