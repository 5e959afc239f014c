"""ctypes binding of libmpx (include/mpx.h) for tests and bench.py.

This is plumbing over the C-ABI, not a second implementation: every call goes
to lib/libmpx.so, and importing this module fails loudly if the library is
missing (there is no CPU fallback — the CPU restatement lives in oracle/ and is
only ever used as a checker).

Reference mapping: see include/mpx.h (each entry point cites the
/root/reference/mpi_perf.c call it replaces).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
# MPX_LIB: load another build of the library (A/B of two builds in tools/)
LIB_PATH = os.environ.get("MPX_LIB") or os.path.join(PKG_ROOT, "lib", "libmpx.so")
HEADER_PATH = os.path.join(os.path.dirname(PKG_ROOT), "include", "mpx.h")

# enum values (include/mpx.h)
OK, ERR_INVALID, ERR_HIP, ERR_NOMEM, ERR_TIMEOUT, ERR_RCCL, ERR_UNSUPPORTED, ERR_STATE, ERR_CHECK = range(9)
ENGINE_KERNEL, ENGINE_SDMA, ENGINE_RCCL = 0, 1, 2
ENGINE_HOST = 3   # reserved: mpx_init refuses it, MPX_ERR_UNSUPPORTED
ENGINES = {"kernel": ENGINE_KERNEL, "sdma": ENGINE_SDMA, "rccl": ENGINE_RCCL}
MODE_PINGPONG, MODE_NONBLOCKING, MODE_UNIDIR = 0, 1, 2
MODES = {"pingpong": MODE_PINGPONG, "nonblocking": MODE_NONBLOCKING, "unidir": MODE_UNIDIR}
FILL_BYTE, FILL_SPLITMIX = 0, 1
XFER_STREAM = 1
XFER_PULL = 2
XFER_NOSTAGE = 4
XFER_FAN_LL = 8      # MPX_FAN_LL (mpx_fan_opts.flags): the lock-step LL fan exchange
FAN_LL_MAX = 4096    # MPX_FAN_LL_MAX: its largest block_len
PROTO_FAN_LL = 10    # mpx_timing.protocol of such a call
PROTO_HOSTLINK_LL = 11     # a host-link call (xfer_hostlink / host_xfer) with LL granules
PROTO_HOSTLINK_BULK = 12   # a host-link call above the LL threshold
PROTO_HOSTLINK_DUPLEX = 13  # the host link's full-duplex loop (xfer_hostlink_duplex / host_xfer_duplex)
HOSTLINK_HEADER_PATH = os.path.join(PKG_ROOT, "csrc", "mpx_hostlink.h")
ABI_VERSION = 7
PATTERN_SEED = 0x6D70695F70657266
MAX_RANKS = 64
RANK_DESC_BYTES = 512
RCCL_ID_BYTES = 128
PROTOCOLS = {0: "ll", 1: "bulk", 2: "sdma", 3: "rccl", 4: "copy", 5: "copy_steps", 6: "copy_pipe", 7: "pull", 8: "sdma_pull",
             9: "fan"}


class Timing(C.Structure):
    _fields_ = [
        ("wall_s", C.c_double),
        ("device_s", C.c_double),
        ("bytes", C.c_uint64),
        ("launches", C.c_int32),
        ("nwg", C.c_int32),
        ("protocol", C.c_int32),
        ("check_failures", C.c_int32),
        ("check_iters", C.c_uint64),
        ("recv_done", C.c_uint64),
        ("recv_digest", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["protocol"] = PROTOCOLS.get(self.protocol, self.protocol)
        return d


class XferOpts(C.Structure):
    _fields_ = [
        ("check", C.c_int32),
        ("flags", C.c_int32),
        ("expect_checksum", C.c_uint64),
        ("expect_ack", C.c_uint64),
        ("timeout_ms", C.c_uint32),
        ("nwg", C.c_int32),
    ]


SEQ_AUTO_MAX = 1 << 28   # MPX_SEQ_AUTO_MAX: bytes xfer_seq generates on the CPU when expect is None


class SeqOpts(C.Structure):
    """mpx_seq_opts (include/mpx_seq.h)"""
    _fields_ = [
        ("seed", C.c_uint64),
        ("check", C.c_int32),
        ("flags", C.c_int32),
        ("timeout_ms", C.c_uint32),
        ("nwg", C.c_int32),
        ("expect", C.POINTER(C.c_uint64)),
    ]


class HostBox(C.Structure):
    """hostlink::HostBox (csrc/mpx_hostlink.h): one direction of a host
    endpoint's mailbox, rows indexed by the GPU peer's rank"""
    _fields_ = [
        ("flag", C.c_uint64 * 256 * 64),
        ("ll", C.c_uint64 * 2048 * 64),
        ("credit", C.c_uint64 * 256 * 64),
        ("posted", C.c_uint64 * 64),
        ("ready", C.c_uint64 * 64),
    ]


class HostMailbox(C.Structure):
    """hostlink::HostMailbox: `in` is written by the GPU, `out` by the CPU"""
    _fields_ = [("in", HostBox), ("out", HostBox)]


class FanOpts(C.Structure):
    """mpx_fan_opts"""
    _fields_ = [
        ("check", C.c_int32),
        ("flags", C.c_int32),
        ("timeout_ms", C.c_uint32),
        ("nwg", C.c_int32),
        ("expect_checksum", C.POINTER(C.c_uint64)),
    ]


class FanSeqOpts(C.Structure):
    """mpx_fan_seq_opts (include/mpx_fan_seq.h)"""
    _fields_ = [
        ("seed", C.c_uint64),
        ("check", C.c_int32),
        ("flags", C.c_int32),
        ("timeout_ms", C.c_uint32),
        ("nwg", C.c_int32),
        ("expect", C.POINTER(C.c_uint64)),
    ]


class FanLink(C.Structure):
    """mpx_fan_link: one link's results of a fan call"""
    _fields_ = [
        ("peer", C.c_int32),
        ("nwg", C.c_int32),
        ("recv_done", C.c_uint64),
        ("recv_digest", C.c_uint64),
        ("check_failures", C.c_int32),
        ("pad", C.c_int32),
        ("device_s", C.c_double),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class Phases(C.Structure):
    _fields_ = ([(k, C.c_double) for k in ("wall_s", "host_prep_s", "launch_to_start_s", "posted_wait_s", "kernel_s",
                                            "done_to_return_s")]
                + [("armed", C.c_int32), ("resident", C.c_int32), ("first_iter_s", C.c_double), ("tail_s", C.c_double)])

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


LAT_BUCKETS = 464
LAT_RAW_MAX = 1 << 22
FAN_LAT_RAW_MAX = 1 << 16   # MPX_FAN_LAT_RAW_MAX: the link recorder's (fan_lat_enable)
HOSTLINK_LAT_RAW_MAX = 1 << 16   # MPX_HOSTLINK_LAT_RAW_MAX: the host-link recorder's (hostlink_lat_enable)


class Lat(C.Structure):
    """mpx_lat: a rank's per-iteration latency distribution (ticks of 10 ns)"""
    _fields_ = ([(k, C.c_uint64) for k in ("count", "calls", "min_ticks", "max_ticks", "sum_ticks", "max_iter",
                                            "last_iters")]
                + [("tick_s", C.c_double), ("hist", C.c_uint32 * LAT_BUCKETS)])

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["hist"] = list(self.hist)
        return d


def lat_bucket(v: int) -> int:
    """mpx_lat_bucket (include/mpx.h): the histogram bucket of v ticks"""
    if v < 32:
        return v
    if v >> 32:
        return LAT_BUCKETS - 1
    e = v.bit_length() - 1
    return 32 + (e - 5) * 16 + ((v >> (e - 4)) & 15)


def lat_bucket_floor(b: int) -> int:
    """mpx_lat_bucket_floor: the smallest value of bucket b"""
    if b < 32:
        return max(b, 0)
    return (16 + (b - 32) % 16) << ((b - 32) // 16 + 1)


def lat_quantile(lat: dict, q: float) -> int:
    """mpx_lat_quantile over a lat_get() dict: ticks"""
    count = lat["count"]
    if count == 0:
        return 0
    x = min(max(q, 0.0), 1.0) * float(count)
    want = int(x)
    if float(want) < x:
        want += 1
    cum, b = 0, 0
    for b in range(LAT_BUCKETS - 1):
        cum += lat["hist"][b]
        if cum >= want:
            break
    else:
        b = LAT_BUCKETS - 1
    return min(max(lat_bucket_floor(b), lat["min_ticks"]), lat["max_ticks"])


def pattern_key(seed: int, src: int, dst: int, it: int) -> int:
    """mpx_pattern_key (include/mpx.h)."""
    return (seed ^ (src << 56) ^ (dst << 48) ^ (it << 24)) & 0xFFFFFFFFFFFFFFFF


_SIGS = {
    "mpx_version": (C.c_int, []),
    "mpx_strerror": (C.c_char_p, [C.c_int]),
    "mpx_last_error": (C.c_char_p, []),
    "mpx_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mpx_link_info": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mpx_device_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "mpx_last_phases": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Phases)]),
    "mpx_init": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mpx_finalize": (C.c_int, [C.c_void_p]),
    "mpx_shutdown": (C.c_int, []),
    "mpx_live_events": (C.c_int, [C.POINTER(C.c_int)]),
    "mpx_link_counters": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "mpx_test_advance_link": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64]),
    "mpx_alloc": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mpx_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mpx_fill": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64]),
    "mpx_checksum": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "mpx_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mpx_copy": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Timing)]),
    "mpx_rank_attach": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "mpx_rank_export": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mpx_rank_import": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mpx_xfer": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                           C.c_int, C.POINTER(C.c_double)]),
    "mpx_xfer_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                              C.c_int, C.POINTER(XferOpts), C.POINTER(Timing)]),
    "mpx_xfer_fan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p,
                               C.c_int, C.c_size_t, C.POINTER(FanOpts), C.POINTER(Timing), C.POINTER(FanLink)]),
    "mpx_fan_width": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mpx_xfer_prepare": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(XferOpts)]),
    "mpx_xfer_arm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_int, C.POINTER(XferOpts)]),
    "mpx_xfer_disarm": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_barrier": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_lat_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mpx_lat_disable": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_lat_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_lat_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Lat)]),
    "mpx_lat_raw": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]),
    "mpx_fan_lat_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mpx_fan_lat_disable": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_fan_lat_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_fan_lat_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Lat)]),
    "mpx_fan_lat_raw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]),
    "mpx_hostlink_lat_enable": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mpx_hostlink_lat_disable": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_hostlink_lat_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "mpx_hostlink_lat_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Lat)]),
    "mpx_hostlink_lat_raw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int)]),
    "mpx_host_attach": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t]),
    "mpx_host_buffers": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mpx_xfer_hostlink": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.POINTER(XferOpts), C.POINTER(Timing)]),
    "mpx_host_xfer": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(XferOpts),
                                C.POINTER(Timing)]),
    "mpx_xfer_hostlink_duplex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                           C.POINTER(XferOpts), C.POINTER(Timing)]),
    "mpx_host_xfer_duplex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(XferOpts),
                                       C.POINTER(Timing)]),
    "mpx_host_checksum": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "mpx_hostlink_ll_max": (C.c_int, []),
    "mpx_xfer_seq": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_int, C.POINTER(SeqOpts), C.POINTER(Timing)]),
    "mpx_seq_expect": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint64)]),
    "mpx_xfer_fan_seq": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_size_t, C.POINTER(FanSeqOpts), C.POINTER(Timing), C.POINTER(FanLink)]),
    "mpx_xfer_hostlink_seq": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.POINTER(SeqOpts), C.POINTER(Timing)]),
    "mpx_host_xfer_seq": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SeqOpts),
                                    C.POINTER(Timing)]),
    "mpx_rccl_version": (C.c_int, [C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "mpx_rccl_get_unique_id": (C.c_int, [C.c_void_p]),
    "mpx_rccl_init_rank": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mpx_rccl_init_all": (C.c_int, [C.c_void_p]),
}

_lib = None


def lib() -> C.CDLL:
    """Load lib/libmpx.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libmpx not built: {LIB_PATH} missing (run __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.mpx_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH}: ABI version {L.mpx_version()}, this binding needs {ABI_VERSION} "
                              "(stale build: run __graft_entry__.build())")
        _lib = L
    return _lib


class MpxError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        L = lib()
        super().__init__(f"{what}: {L.mpx_strerror(status).decode()} ({L.mpx_last_error().decode()})")


def check(status: int, what: str) -> None:
    if status != OK:
        raise MpxError(status, what)


def device_count() -> int:
    n = C.c_int(0)
    check(lib().mpx_device_count(C.byref(n)), "mpx_device_count")
    return n.value


LINK_TYPES = {0: "hypertransport", 1: "qpi", 2: "pcie", 3: "infiniband", 4: "xgmi"}


def link_info(dev_a: int, dev_b: int) -> dict:
    """mpx_link_info: the interconnect between two visible GPUs."""
    t, h = C.c_int(0), C.c_int(0)
    check(lib().mpx_link_info(dev_a, dev_b, C.byref(t), C.byref(h)), "mpx_link_info")
    return {"type": LINK_TYPES.get(t.value, t.value), "hops": h.value}


def fan_width(nranks: int, block_len: int, same_device: bool = True, nwg: int = 0) -> int:
    """mpx_fan_width: the width mpx_xfer_fan gives a link (-1: refused)"""
    return lib().mpx_fan_width(nranks, block_len, 1 if same_device else 0, nwg)


def host_checksum(data, offset: int = 0, n: int | None = None) -> int:
    """mpx_host_checksum: mpx_checksum's value of n bytes of `data` (bytes, or
    any writable buffer such as host_buffers' arrays) from `offset`, on the CPU"""
    if isinstance(data, (bytes, bytearray)):
        buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
        size = len(data)
    else:
        buf = (C.c_ubyte * max(len(data), 1)).from_buffer(data)
        size = len(data)
    if n is None:
        n = size - offset
    if offset < 0 or n < 0 or offset + n > size:
        raise ValueError("host_checksum: range outside the data")
    out = C.c_uint64()
    check(lib().mpx_host_checksum(C.c_void_p(C.addressof(buf) + offset), n, C.byref(out)), "mpx_host_checksum")
    return out.value


def hostlink_ll_max() -> int:
    """mpx_hostlink_ll_max: the host link's LL threshold in force (MPX_HOSTLINK_LL)"""
    return lib().mpx_hostlink_ll_max()


def seq_expect(seed: int, src: int, dst: int, it: int, n: int) -> int:
    """mpx_seq_expect: the checksum of the n-byte payload rank src sends rank
    dst in iteration `it` of a sequenced call (xfer_seq), on the CPU"""
    out = C.c_uint64()
    check(lib().mpx_seq_expect(seed & 0xFFFFFFFFFFFFFFFF, src, dst, it, n, C.byref(out)), "mpx_seq_expect")
    return out.value


def shutdown() -> None:
    """mpx_shutdown: destroy the pooled rank streams (no context alive)."""
    check(lib().mpx_shutdown(), "mpx_shutdown")


def live_events() -> int:
    """mpx_live_events: HIP events libmpx holds right now (leak check)."""
    n = C.c_int(0)
    check(lib().mpx_live_events(C.byref(n)), "mpx_live_events")
    return n.value


def bus_id(dev: int) -> str:
    """mpx_device_bus_id: the GPU's PCI bus id, "DDDD:BB:DD.F"."""
    buf = C.create_string_buffer(64)
    check(lib().mpx_device_bus_id(dev, buf, 64), "mpx_device_bus_id")
    return buf.value.decode()


@dataclass
class Buffer:
    ptr: int
    dev: int
    size: int


class Context:
    """Thin object wrapper of an mpx_ctx."""

    def __init__(self, nranks: int, engine: int | str = ENGINE_KERNEL):
        if isinstance(engine, str):
            engine = ENGINES[engine]
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.mpx_init(nranks, engine, C.byref(self.h)), "mpx_init")
        self.nranks = nranks
        self.engine = engine
        self._lat_cap = {}   # rank -> raw_cap of its latency recorder (lat_enable)
        self._fan_lat_cap = {}   # rank -> raw_cap of its link recorder (fan_lat_enable)
        self._hostlink_lat_cap = {}   # rank -> raw_cap of its host-link recorder (hostlink_lat_enable)
        self._host_len = {}      # host endpoint -> its attached length (host_attach)

    def close(self) -> None:
        if self.h:
            check(self.L.mpx_finalize(self.h), "mpx_finalize")
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # buffers
    def alloc(self, dev: int, size: int) -> Buffer:
        p = C.c_void_p()
        check(self.L.mpx_alloc(self.h, dev, size, C.byref(p)), "mpx_alloc")
        return Buffer(p.value, dev, size)

    def free(self, b: Buffer) -> None:
        check(self.L.mpx_free(self.h, C.c_void_p(b.ptr)), "mpx_free")

    def fill(self, b: Buffer, n: int, pattern: int, arg: int) -> None:
        check(self.L.mpx_fill(self.h, b.dev, C.c_void_p(b.ptr), n, pattern, arg & 0xFFFFFFFFFFFFFFFF), "mpx_fill")

    def checksum(self, b: Buffer, n: int, offset: int = 0) -> int:
        out = C.c_uint64()
        check(self.L.mpx_checksum(self.h, b.dev, C.c_void_p(b.ptr + offset), n, C.byref(out)), "mpx_checksum")
        return out.value

    def read(self, b: Buffer, n: int, offset: int = 0) -> bytes:
        buf = C.create_string_buffer(max(n, 1))
        check(self.L.mpx_read(self.h, b.dev, buf, C.c_void_p(b.ptr + offset), n), "mpx_read")
        return buf.raw[:n]

    def copy(self, dev: int, dst: Buffer, src: Buffer, n: int, iters: int) -> Timing:
        t = Timing()
        check(self.L.mpx_copy(self.h, dev, C.c_void_p(dst.ptr), C.c_void_p(src.ptr), n, iters, C.byref(t)), "mpx_copy")
        return t

    # ranks
    def attach(self, rank: int, dev: int, tx: Buffer, rx: Buffer, length: int) -> None:
        check(self.L.mpx_rank_attach(self.h, rank, dev, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr), length),
              "mpx_rank_attach")

    def export(self, rank: int) -> bytes:
        buf = C.create_string_buffer(RANK_DESC_BYTES)
        check(self.L.mpx_rank_export(self.h, rank, buf), "mpx_rank_export")
        return buf.raw

    def import_rank(self, rank: int, desc: bytes) -> None:
        buf = C.create_string_buffer(bytes(desc), RANK_DESC_BYTES)
        check(self.L.mpx_rank_import(self.h, rank, buf), "mpx_rank_import")

    def xfer(self, mode: int, group: int, my_rank: int, peer_rank: int, iters: int, tx: Buffer, rx: Buffer,
             length: int, check_payload: bool = False, expect: int = 0, expect_ack: int = 0,
             timeout_ms: int = 0, nwg: int = 0, stream: bool = False, pull: bool = False,
             stage: bool = True, after=None) -> Timing:
        """mpx_xfer_ex.  after: a spin barrier (mpx.spin.SpinBarrier) to wait
        on first, from C, so the call starts right as the barrier opens"""
        flags = (XFER_STREAM if stream else 0) | (XFER_PULL if pull else 0) | (0 if stage else XFER_NOSTAGE)
        o = XferOpts(check=1 if check_payload else 0, flags=flags, expect_checksum=expect,
                     expect_ack=expect_ack, timeout_ms=timeout_ms, nwg=nwg)
        t = Timing()
        if after is not None:
            st = after.wait_then(C.cast(self.L.mpx_xfer_ex, C.c_void_p), self.h, mode, group, my_rank, peer_rank,
                                 iters, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr), length, C.byref(o), C.byref(t))
        else:
            st = self.L.mpx_xfer_ex(self.h, mode, group, my_rank, peer_rank, iters, C.c_void_p(tx.ptr),
                                    C.c_void_p(rx.ptr), length, C.byref(o), C.byref(t))
        check(st, "mpx_xfer_ex")
        return t

    def xfer_seq(self, mode: int, group: int, my_rank: int, peer_rank: int, iters: int, tx: Buffer, rx: Buffer,
                 length: int, seed: int, check_payload: bool = False, expect=None, timeout_ms: int = 0, nwg: int = 0,
                 stream: bool = False) -> Timing:
        """mpx_xfer_seq: the pair loop with a generated payload of its own in
        every iteration.  expect: check mode, the checksum of each of the
        `iters` payloads this side receives (None: the library computes
        them).  A failing call raises MpxError carrying .timing"""
        arr = None
        if expect is not None:
            expect = list(expect)
            arr = (C.c_uint64 * max(len(expect), 1))(*expect)
        o = SeqOpts(seed=seed & 0xFFFFFFFFFFFFFFFF, check=1 if check_payload else 0, flags=XFER_STREAM if stream else 0,
                    timeout_ms=timeout_ms, nwg=nwg,
                    expect=C.cast(arr, C.POINTER(C.c_uint64)) if arr is not None else None)
        t = Timing()
        st = self.L.mpx_xfer_seq(self.h, mode, group, my_rank, peer_rank, iters, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr),
                                 length, C.byref(o), C.byref(t))
        if st != OK:
            e = MpxError(st, "mpx_xfer_seq")
            e.timing = t
            raise e
        return t

    def fan(self, my_rank: int, peers, iters: int, tx: Buffer, rx: Buffer, block_len: int, stride: int,
            check_payload: bool = False, expect=None, timeout_ms: int = 0, nwg: int = 0, stream: bool = False,
            ll: bool = False):
        """mpx_xfer_fan: my_rank exchanges block_len bytes with every rank of
        `peers` in one launch (block j of tx / rx at j * stride).  expect:
        check mode, the checksum of each peer's block for my_rank, in the
        order of `peers`.  ll: MPX_FAN_LL, per link a lock-step exchange of LL
        granules (block_len <= FAN_LL_MAX).  Returns (Timing, [link dicts]); a failing call
        raises MpxError carrying .timing and .links as far as they were
        filled."""
        peers = list(peers)
        n = len(peers)
        arr = (C.c_int * max(n, 1))(*peers)
        exp = (C.c_uint64 * max(n, 1))(*(list(expect) if expect is not None else [0] * n))
        flags = (XFER_STREAM if stream else 0) | (XFER_FAN_LL if ll else 0)
        o = FanOpts(check=1 if check_payload else 0, flags=flags, timeout_ms=timeout_ms,
                    nwg=nwg, expect_checksum=C.cast(exp, C.POINTER(C.c_uint64)))
        t = Timing()
        links = (FanLink * max(n, 1))()
        st = self.L.mpx_xfer_fan(self.h, my_rank, n, arr, iters, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr), block_len,
                                 stride, C.byref(o), C.byref(t), links)
        out = [links[k].as_dict() for k in range(n)]
        if st != OK:
            e = MpxError(st, "mpx_xfer_fan")
            e.timing, e.links = t, out
            raise e
        return t, out

    def xfer_fan_seq(self, my_rank: int, peers, iters: int, tx: Buffer, rx: Buffer, block_len: int, stride: int,
                     seed: int, check_payload: bool = False, expect=None, timeout_ms: int = 0, nwg: int = 0,
                     stream: bool = False, ll: bool = False):
        """mpx_xfer_fan_seq: the fan exchange (arguments as fan) with a
        generated payload per (sender, receiver, iteration); tx is not sent.
        expect: check mode, the checksums of the payloads this rank receives,
        expect[k * iters + i] for peers[k] (None: the library computes them).
        Returns (Timing, [link dicts]); a failing call raises MpxError
        carrying .timing and .links as far as they were filled."""
        peers = list(peers)
        n = len(peers)
        arr = (C.c_int * max(n, 1))(*peers)
        exp = None
        if expect is not None:
            expect = list(expect)
            exp = (C.c_uint64 * max(len(expect), 1))(*expect)
        flags = (XFER_STREAM if stream else 0) | (XFER_FAN_LL if ll else 0)
        o = FanSeqOpts(seed=seed & 0xFFFFFFFFFFFFFFFF, check=1 if check_payload else 0, flags=flags,
                       timeout_ms=timeout_ms, nwg=nwg,
                       expect=C.cast(exp, C.POINTER(C.c_uint64)) if exp is not None else None)
        t = Timing()
        links = (FanLink * max(n, 1))()
        st = self.L.mpx_xfer_fan_seq(self.h, my_rank, n, arr, iters, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr), block_len,
                                     stride, C.byref(o), C.byref(t), links)
        out = [links[k].as_dict() for k in range(n)]
        if st != OK:
            e = MpxError(st, "mpx_xfer_fan_seq")
            e.timing, e.links = t, out
            raise e
        return t, out

    # host link (include/mpx_hostlink.h)
    def host_attach(self, rank: int, length: int) -> None:
        """mpx_host_attach: make `rank` a host endpoint with pinned tx / rx of `length` bytes"""
        check(self.L.mpx_host_attach(self.h, rank, length), "mpx_host_attach")
        self._host_len[rank] = length

    def host_buffers(self, rank: int):
        """mpx_host_buffers: the endpoint's (tx, rx) as writable ctypes byte
        arrays over its pinned memory (valid until close)"""
        tx, rx = C.c_void_p(), C.c_void_p()
        check(self.L.mpx_host_buffers(self.h, rank, C.byref(tx), C.byref(rx)), "mpx_host_buffers")
        n = max(self._host_len[rank], 16)
        return (C.c_ubyte * n).from_address(tx.value), (C.c_ubyte * n).from_address(rx.value)

    def _hostlink_opts(self, check_payload, expect, expect_ack, timeout_ms, nwg, stage) -> XferOpts:
        return XferOpts(check=1 if check_payload else 0, flags=0 if stage else XFER_NOSTAGE, expect_checksum=expect,
                        expect_ack=expect_ack, timeout_ms=timeout_ms, nwg=nwg)

    def xfer_hostlink(self, mode: int, group: int, my_rank: int, host_rank: int, iters: int, tx: Buffer, rx: Buffer,
                      length: int, check_payload: bool = False, expect: int = 0, expect_ack: int = 0,
                      timeout_ms: int = 0, nwg: int = 0, stage: bool = True) -> Timing:
        """mpx_xfer_hostlink: GPU rank my_rank's side of the loop with host
        endpoint host_rank.  A failing call raises MpxError carrying .timing"""
        o = self._hostlink_opts(check_payload, expect, expect_ack, timeout_ms, nwg, stage)
        t = Timing()
        st = self.L.mpx_xfer_hostlink(self.h, mode, group, my_rank, host_rank, iters, C.c_void_p(tx.ptr),
                                      C.c_void_p(rx.ptr), length, C.byref(o), C.byref(t))
        if st != OK:
            e = MpxError(st, "mpx_xfer_hostlink")
            e.timing = t
            raise e
        return t

    def host_xfer(self, mode: int, group: int, host_rank: int, peer_rank: int, iters: int, length: int,
                  check_payload: bool = False, expect: int = 0, expect_ack: int = 0, timeout_ms: int = 0,
                  nwg: int = 0) -> Timing:
        """mpx_host_xfer: host endpoint host_rank's side of the same loop, on
        the calling thread (ctypes releases the GIL for the call)"""
        o = self._hostlink_opts(check_payload, expect, expect_ack, timeout_ms, nwg, True)
        t = Timing()
        st = self.L.mpx_host_xfer(self.h, mode, group, host_rank, peer_rank, iters, length, C.byref(o), C.byref(t))
        if st != OK:
            e = MpxError(st, "mpx_host_xfer")
            e.timing = t
            raise e
        return t

    # host link, sequenced payloads (include/mpx_hostlink_seq.h)
    @staticmethod
    def _seq_opts(seed, check_payload, expect, timeout_ms, nwg, flags=0):
        arr = None
        if expect is not None:
            expect = list(expect)
            arr = (C.c_uint64 * max(len(expect), 1))(*expect)
        o = SeqOpts(seed=seed & 0xFFFFFFFFFFFFFFFF, check=1 if check_payload else 0, flags=flags, timeout_ms=timeout_ms,
                    nwg=nwg, expect=C.cast(arr, C.POINTER(C.c_uint64)) if arr is not None else None)
        return o, arr   # (arr: kept alive by the caller for the call)

    def xfer_hostlink_seq(self, mode: int, group: int, my_rank: int, host_rank: int, iters: int, tx: Buffer, rx: Buffer,
                          length: int, seed: int, check_payload: bool = False, expect=None, timeout_ms: int = 0,
                          nwg: int = 0, flags: int = 0) -> Timing:
        """mpx_xfer_hostlink_seq: GPU rank my_rank's side of the host-link loop
        with a generated payload of its own in every iteration.  expect: check
        mode, the checksum of each of the `iters` payloads this side receives
        (None: the library computes them).  A failing call raises MpxError
        carrying .timing"""
        o, keep = self._seq_opts(seed, check_payload, expect, timeout_ms, nwg, flags)
        t = Timing()
        st = self.L.mpx_xfer_hostlink_seq(self.h, mode, group, my_rank, host_rank, iters, C.c_void_p(tx.ptr),
                                          C.c_void_p(rx.ptr), length, C.byref(o), C.byref(t))
        del keep
        if st != OK:
            e = MpxError(st, "mpx_xfer_hostlink_seq")
            e.timing = t
            raise e
        return t

    def host_xfer_seq(self, mode: int, group: int, host_rank: int, peer_rank: int, iters: int, length: int, seed: int,
                      check_payload: bool = False, expect=None, timeout_ms: int = 0, nwg: int = 0,
                      flags: int = 0) -> Timing:
        """mpx_host_xfer_seq: host endpoint host_rank's side of the same loop,
        on the calling thread; a bulk send writes each payload into the
        endpoint's tx"""
        o, keep = self._seq_opts(seed, check_payload, expect, timeout_ms, nwg, flags)
        t = Timing()
        st = self.L.mpx_host_xfer_seq(self.h, mode, group, host_rank, peer_rank, iters, length, C.byref(o), C.byref(t))
        del keep
        if st != OK:
            e = MpxError(st, "mpx_host_xfer_seq")
            e.timing = t
            raise e
        return t

    # host link, the full-duplex non-blocking loop (include/mpx_hostlink_duplex.h)
    def xfer_hostlink_duplex(self, my_rank: int, host_rank: int, iters: int, tx: Buffer, rx: Buffer, length: int,
                             check_payload: bool = False, expect: int = 0, timeout_ms: int = 0, nwg: int = 0,
                             stage: bool = True) -> Timing:
        """mpx_xfer_hostlink_duplex: GPU rank my_rank's side of the non-blocking
        loop with host endpoint host_rank (nwg: per direction).  A failing
        call raises MpxError carrying .timing"""
        o = self._hostlink_opts(check_payload, expect, 0, timeout_ms, nwg, stage)
        t = Timing()
        st = self.L.mpx_xfer_hostlink_duplex(self.h, my_rank, host_rank, iters, C.c_void_p(tx.ptr), C.c_void_p(rx.ptr),
                                             length, C.byref(o), C.byref(t))
        if st != OK:
            e = MpxError(st, "mpx_xfer_hostlink_duplex")
            e.timing = t
            raise e
        return t

    def host_xfer_duplex(self, host_rank: int, peer_rank: int, iters: int, length: int, check_payload: bool = False,
                         expect: int = 0, timeout_ms: int = 0, nwg: int = 0) -> Timing:
        """mpx_host_xfer_duplex: host endpoint host_rank's side of the same
        loop, on the calling thread (ctypes releases the GIL for the call)"""
        o = self._hostlink_opts(check_payload, expect, 0, timeout_ms, nwg, True)
        t = Timing()
        st = self.L.mpx_host_xfer_duplex(self.h, host_rank, peer_rank, iters, length, C.byref(o), C.byref(t))
        if st != OK:
            e = MpxError(st, "mpx_host_xfer_duplex")
            e.timing = t
            raise e
        return t

    def arm(self, mode: int, group: int, my_rank: int, peer_rank: int, iters: int, tx: Buffer, rx: Buffer,
            length: int, check_payload: bool = False, expect: int = 0, expect_ack: int = 0, timeout_ms: int = 0,
            nwg: int = 0, stream: bool = False, pull: bool = False, stage: bool = True) -> None:
        """mpx_xfer_arm: launch the next xfer with these arguments now; the
        xfer call with the same arguments starts it (kernel engine)"""
        flags = (XFER_STREAM if stream else 0) | (XFER_PULL if pull else 0) | (0 if stage else XFER_NOSTAGE)
        o = XferOpts(check=1 if check_payload else 0, flags=flags, expect_checksum=expect,
                     expect_ack=expect_ack, timeout_ms=timeout_ms, nwg=nwg)
        check(self.L.mpx_xfer_arm(self.h, mode, group, my_rank, peer_rank, iters, C.c_void_p(tx.ptr),
                                  C.c_void_p(rx.ptr), length, C.byref(o)), "mpx_xfer_arm")

    def disarm(self, rank: int) -> None:
        check(self.L.mpx_xfer_disarm(self.h, rank), "mpx_xfer_disarm")

    def prepare(self, mode: int, group: int, my_rank: int, peer_rank: int, iters: int, length: int,
                timeout_ms: int = 0, pull: bool = False) -> None:
        """mpx_xfer_prepare: before timing, build the SDMA engine's graph chunks
        (pull: its pulled form's) or set up the RCCL engine's channel to
        peer_rank (both ranks call it)"""
        o = XferOpts(timeout_ms=timeout_ms, flags=XFER_PULL if pull else 0)
        check(self.L.mpx_xfer_prepare(self.h, mode, group, my_rank, peer_rank, iters, length, C.byref(o)),
              "mpx_xfer_prepare")

    def phases(self, rank: int) -> dict:
        """mpx_last_phases: where rank's last kernel-engine call spent its time"""
        p = Phases()
        check(self.L.mpx_last_phases(self.h, rank, C.byref(p)), "mpx_last_phases")
        return p.as_dict()

    def link_counters(self, my_rank: int, peer_rank: int) -> dict:
        """mpx_link_counters: the link's push and call counters and my_rank's
        token, as whole 64-bit numbers"""
        out = (C.c_uint64 * 4)()
        check(self.L.mpx_link_counters(self.h, my_rank, peer_rank, out), "mpx_link_counters")
        return dict(tx_seq=int(out[0]), rx_seq=int(out[1]), calls=int(out[2]), token=int(out[3]))

    def test_advance_link(self, my_rank: int, peer_rank: int, seq_by: int = 0, calls_by: int = 0,
                          token_by: int = 0) -> None:
        """mpx_test_advance_link (test only, MPX_TEST gate): the counters jump
        forward; both ranks of a link alike"""
        check(self.L.mpx_test_advance_link(self.h, my_rank, peer_rank, seq_by, calls_by, token_by),
              "mpx_test_advance_link")

    # the two latency recorders' reads: `key` is (rank,) or (rank, peer)
    def _lat_dict(self, fn: str, *key: int) -> dict:
        l = Lat()
        check(getattr(self.L, fn)(self.h, *key, C.byref(l)), fn)
        return l.as_dict()

    def _lat_stamps(self, fn: str, caps: dict, cap: int | None, *key: int) -> list[int]:
        if cap is None:
            cap = caps.get(key[0], 0) + 1
        n = C.c_int(0)
        buf = (C.c_uint64 * max(cap, 1))()
        check(getattr(self.L, fn)(self.h, *key, buf, cap, C.byref(n)), fn)
        return list(buf[:n.value])

    # per-iteration latency recorder (kernel engine)
    def lat_enable(self, rank: int, raw_cap: int = 0) -> None:
        """mpx_lat_enable: trace rank's ping-pong / unidir calls from now on,
        keeping the first raw_cap iterations' stamps of each call; resets"""
        check(self.L.mpx_lat_enable(self.h, rank, raw_cap), "mpx_lat_enable")
        self._lat_cap[rank] = raw_cap

    def lat_disable(self, rank: int) -> None:
        check(self.L.mpx_lat_disable(self.h, rank), "mpx_lat_disable")

    def lat_reset(self, rank: int) -> None:
        check(self.L.mpx_lat_reset(self.h, rank), "mpx_lat_reset")

    def lat_get(self, rank: int) -> dict:
        """mpx_lat_get: the distribution accumulated since enable / reset"""
        return self._lat_dict("mpx_lat_get", rank)

    def lat_raw(self, rank: int, cap: int | None = None) -> list[int]:
        """mpx_lat_raw: the last traced call's stamps t[0 .. min(iters, raw_cap)]
        (cap: at most that many; default all of them)"""
        return self._lat_stamps("mpx_lat_raw", self._lat_cap, cap, rank)

    # per-link latency recorder of the lock-step LL fan exchange (kernel engine)
    def fan_lat_enable(self, rank: int, raw_cap: int = 0) -> None:
        """mpx_fan_lat_enable: trace every link of rank's MPX_FAN_LL calls from
        now on, keeping the first raw_cap iterations' stamps per link; resets"""
        check(self.L.mpx_fan_lat_enable(self.h, rank, raw_cap), "mpx_fan_lat_enable")
        self._fan_lat_cap[rank] = raw_cap

    def fan_lat_disable(self, rank: int) -> None:
        check(self.L.mpx_fan_lat_disable(self.h, rank), "mpx_fan_lat_disable")

    def fan_lat_reset(self, rank: int) -> None:
        check(self.L.mpx_fan_lat_reset(self.h, rank), "mpx_fan_lat_reset")

    def fan_lat_get(self, rank: int, peer: int) -> dict:
        """mpx_fan_lat_get: link (rank, peer)'s distribution since enable /
        reset (the dict of lat_get; blocks are keyed by the peer's rank)"""
        return self._lat_dict("mpx_fan_lat_get", rank, peer)

    def fan_lat_raw(self, rank: int, peer: int, cap: int | None = None) -> list[int]:
        """mpx_fan_lat_raw: link (rank, peer)'s stamps t[0 .. min(iters, raw_cap)]
        of the last traced call that listed peer (cap: at most that many)"""
        return self._lat_stamps("mpx_fan_lat_raw", self._fan_lat_cap, cap, rank, peer)

    # host-link recorder (include/mpx_hostlink_lat.h): rank is a GPU rank or a host endpoint
    def hostlink_lat_enable(self, rank: int, raw_cap: int = 0) -> None:
        """mpx_hostlink_lat_enable: trace every host-link call of rank (a GPU
        rank: xfer_hostlink; an endpoint: host_xfer) from now on, per peer,
        keeping the first raw_cap iterations' stamps of each call; resets"""
        check(self.L.mpx_hostlink_lat_enable(self.h, rank, raw_cap), "mpx_hostlink_lat_enable")
        self._hostlink_lat_cap[rank] = raw_cap

    def hostlink_lat_disable(self, rank: int) -> None:
        check(self.L.mpx_hostlink_lat_disable(self.h, rank), "mpx_hostlink_lat_disable")

    def hostlink_lat_reset(self, rank: int) -> None:
        check(self.L.mpx_hostlink_lat_reset(self.h, rank), "mpx_hostlink_lat_reset")

    def hostlink_lat_get(self, rank: int, peer: int) -> dict:
        """mpx_hostlink_lat_get: link (rank, peer)'s distribution since enable /
        reset (the dict of lat_get; tick_s is 1e-8 on a GPU rank, 1e-9 on an endpoint)"""
        return self._lat_dict("mpx_hostlink_lat_get", rank, peer)

    def hostlink_lat_raw(self, rank: int, peer: int, cap: int | None = None) -> list[int]:
        """mpx_hostlink_lat_raw: link (rank, peer)'s stamps t[0 .. min(iters, raw_cap)]
        of the last traced call with that peer (cap: at most that many)"""
        return self._lat_stamps("mpx_hostlink_lat_raw", self._hostlink_lat_cap, cap, rank, peer)

    def rccl_init_all(self) -> None:
        check(self.L.mpx_rccl_init_all(self.h), "mpx_rccl_init_all")

    def rccl_init_rank(self, rank: int, nranks: int, uid: bytes) -> None:
        buf = C.create_string_buffer(bytes(uid), RCCL_ID_BYTES)
        check(self.L.mpx_rccl_init_rank(self.h, rank, nranks, buf), "mpx_rccl_init_rank")


def rccl_version() -> dict:
    """mpx_rccl_version: the RCCL this process runs and where it came from"""
    v, buf = C.c_int(0), C.create_string_buffer(512)
    check(lib().mpx_rccl_version(C.byref(v), buf, 512), "mpx_rccl_version")
    x = v.value
    return {"version": x, "release": f"{x // 10000}.{x // 100 % 100}.{x % 100}", "library": buf.value.decode()}


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(RCCL_ID_BYTES)
    check(lib().mpx_rccl_get_unique_id(buf), "mpx_rccl_get_unique_id")
    return buf.raw


def header_symbols(path: str = HEADER_PATH) -> list[str]:
    """Every function name include/mpx.h declares (for the export test)."""
    import re

    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?[a-z_]+\s*\*?\s*(mpx_[a-z_0-9]+)\s*\(", txt, flags=re.M)
    return sorted(set(n for n in names if n != "mpx_pattern_key"))
