// mpx_engine_hostlink.hip — the host link (include/mpx_hostlink.h): host
// endpoints (mpx_host_attach, mpx_host_buffers), the GPU side of a host-link
// call (mpx_xfer_hostlink: the arguments of k_xfer_hostlink, launched through
// the kernel engine's one call lifecycle, run_hostlink_kernel) and the CPU
// side (mpx_host_xfer: mpx_hostlink.h's run() on the calling thread); and the
// full-duplex loop's two entry points (include/mpx_hostlink_duplex.h:
// k_hostlink_duplex through run_hostlink_duplex_kernel, run_duplex()).
#include "mpx_runtime.h"

#include "mpx_hostlink.h"

#include <vector>

using namespace mpx;

namespace mpx {
namespace {

using hostlink::HostBox;
using hostlink::HostMailbox;

// the kernels address an endpoint's boxes as device mailboxes
static_assert(hostlink::kRanks == MPX_MAX_RANKS && hostlink::kWG == kMaxPushWG && hostlink::kLLBytes == kLLMaxBytes &&
                  hostlink::kMinChunk == kMinPushChunk,
              "mpx_hostlink.h restates mpx_internal.h's limits");
static_assert(sizeof(HostBox) == sizeof(Mailbox) && offsetof(HostBox, flag) == offsetof(Mailbox, flag) &&
                  offsetof(HostBox, ll) == offsetof(Mailbox, ll) && offsetof(HostBox, credit) == offsetof(Mailbox, credit) &&
                  offsetof(HostBox, posted) == offsetof(Mailbox, posted) && offsetof(HostBox, ready) == offsetof(Mailbox, ready),
              "HostBox has the device mailbox's layout");

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    char* end = nullptr;
    const long x = strtol(v, &end, 10);
    if (*end || x < -0x7fffffffl || x > 0x7fffffffl) return dflt;
    return (int)x;
}

// The width of a host link: the call's option, else MPX_HOSTLINK_WG, else the
// pair rule's 32 KiB per workgroup up to kDefaultMaxWG workgroups (the width
// sweep of tools/hostlink_probe.py: a few workgroups fill the link, and the
// pair rule's 128 at 4 MiB was slower in both directions); narrowed like a
// pair's.  Only things both ends see go in.
int hostlink_nwg(const mpx_xfer_opts* o, long long len) {
    const int env = env_int("MPX_HOSTLINK_WG", 0);
    const int rule = bulk_nwg(len, false);
    return link_nwg((o && o->nwg > 0) ? o->nwg : 0, env > 0 ? env : 0,
                    rule < hostlink::kDefaultMaxWG ? rule : hostlink::kDefaultMaxWG, len);
}

// The checks both sides share, in the header's order.  gpu_rank / host_rank:
// the two ends, whoever calls.
int check_hostlink(mpx_ctx* ctx, int mode, int group, int gpu_rank, int host_rank, int iters, int buff_len,
                   const mpx_xfer_opts* o) {
    if (ctx->engine != MPX_ENGINE_KERNEL) return fail(MPX_ERR_UNSUPPORTED, "the host link: the kernel engine only");
    if (mode == MPX_MODE_NONBLOCKING)
        return fail(MPX_ERR_UNSUPPORTED, "the host link runs the ping-pong and unidir loops only");
    if (mode != MPX_MODE_PINGPONG && mode != MPX_MODE_UNIDIR) return fail(MPX_ERR_INVALID, "mode %d", mode);
    if (group != 0 && group != 1) return fail(MPX_ERR_INVALID, "group %d", group);
    if (gpu_rank < 0 || gpu_rank >= ctx->nranks || host_rank < 0 || host_rank >= ctx->nranks)
        return fail(MPX_ERR_INVALID, "ranks %d/%d", gpu_rank, host_rank);
    if (iters < 0 || buff_len < 0) return fail(MPX_ERR_INVALID, "iters %d, buff_len %d", iters, buff_len);
    const Rank& g = ctx->r[gpu_rank];
    const Rank& h = ctx->r[host_rank];
    if (!h.host) return fail(MPX_ERR_INVALID, "rank %d is not a host endpoint (mpx_host_attach)", host_rank);
    if (!g.local) return fail(MPX_ERR_INVALID, "rank %d is not an attached local GPU rank", gpu_rank);
    if ((size_t)buff_len > g.len || (size_t)buff_len > h.len)
        return fail(MPX_ERR_INVALID, "buff_len %d exceeds an attached length (%zu, %zu)", buff_len, g.len, h.len);
    if (o && (o->flags & ~MPX_XFER_NOSTAGE))
        return fail(MPX_ERR_INVALID, "flags %#x: a host-link call takes MPX_XFER_NOSTAGE only", o->flags);
    if (hostlink_nwg(o, buff_len) < 1) return fail(MPX_ERR_INVALID, "nwg > %d", kMaxPushWG);
    return MPX_OK;
}

}  // namespace

void free_host_endpoint(Rank& rk) {
    if (rk.tx) (void)hipHostFree(rk.tx);
    if (rk.rx) (void)hipHostFree(rk.rx);
    if (rk.host_mb) (void)hipHostFree(rk.host_mb);
    free(rk.host_lat);
    rk.host_lat = nullptr;
    rk.host_lat_on = false;
    rk.tx = rk.rx = nullptr;
    rk.host_mb = nullptr;
    rk.host = false;
}

}  // namespace mpx

extern "C" {

int mpx_hostlink_ll_max(void) {
    const int v = env_int("MPX_HOSTLINK_LL", -1);
    return (v < 0 || v > kLLMaxBytes) ? hostlink::kDefaultLL : v;
}

int mpx_host_checksum(const void* p, size_t n, uint64_t* out) {
    if (!out || (!p && n)) return fail(MPX_ERR_INVALID, "NULL argument");
    *out = hostlink::checksum(p, n);
    return MPX_OK;
}

int mpx_host_attach(mpx_ctx* ctx, int rank, size_t len) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (ctx->engine != MPX_ENGINE_KERNEL) return fail(MPX_ERR_UNSUPPORTED, "mpx_host_attach: the kernel engine only");
    if (rank < 0 || rank >= ctx->nranks) return fail(MPX_ERR_INVALID, "rank %d not in [0,%d)", rank, ctx->nranks);
    if (len > 0x7fffffffull) return fail(MPX_ERR_INVALID, "len %zu exceeds the reference's int buff_len", len);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ctx->r[rank].local || ctx->r[rank].imported || ctx->r[rank].host)
            return fail(MPX_ERR_STATE, "rank %d already registered", rank);
    }
    // The memory kind of Status: host memory mapped into every GPU's address
    // space, coherent (the kernels' sc0 sc1 stores and loads go to memory).
    const unsigned flags = hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable;
    const size_t bytes = len ? len : 16;
    void* p[3] = {nullptr, nullptr, nullptr};
    void* d[3] = {nullptr, nullptr, nullptr};
    const size_t want[3] = {bytes, bytes, sizeof(hostlink::HostMailbox)};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && e == hipSuccess; ++k) {
        e = hipHostMalloc(&p[k], want[k], flags);
        if (e == hipSuccess) {
            memset(p[k], 0, want[k]);
            e = hipHostGetDevicePointer(&d[k], p[k], 0);
        }
    }
    if (e != hipSuccess) {
        for (int k = 0; k < 3; ++k)
            if (p[k]) (void)hipHostFree(p[k]);
        if (e == hipErrorOutOfMemory) return fail(MPX_ERR_NOMEM, "hipHostMalloc(%zu)", bytes);
        HIPCK(e);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Rank& rk = ctx->r[rank];
    if (rk.local || rk.imported || rk.host) {
        for (int k = 0; k < 3; ++k) (void)hipHostFree(p[k]);
        return fail(MPX_ERR_STATE, "rank %d already registered", rank);
    }
    rk.tx = static_cast<unsigned char*>(p[0]);
    rk.rx = static_cast<unsigned char*>(p[1]);
    rk.host_mb = p[2];
    rk.host_tx_dev = static_cast<unsigned char*>(d[0]);
    rk.host_rx_dev = static_cast<unsigned char*>(d[1]);
    rk.host_mb_dev = d[2];
    rk.len = len;
    rk.host = true;
    return MPX_OK;
}

int mpx_host_buffers(mpx_ctx* ctx, int rank, void** tx, void** rx) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (rank < 0 || rank >= ctx->nranks || !ctx->r[rank].host)
        return fail(MPX_ERR_INVALID, "rank %d is not a host endpoint", rank);
    if (tx) *tx = ctx->r[rank].tx;
    if (rx) *rx = ctx->r[rank].rx;
    return MPX_OK;
}

namespace {

// A sequenced host-link call (include/mpx_hostlink_seq.h) beside the ordinary
// one's options: the link's two key bases and, in check mode, the checksum
// of every payload this side receives.
struct SeqCall {
    u64 tx_key, rx_key;
    const uint64_t* want;
};

// The refusals a sequenced call adds to check_hostlink's, and the ordinary
// options it runs under (no flag: nothing reads tx, so nothing is staged)
int check_hostlink_seq(mpx_ctx* ctx, int mode, int group, int gpu_rank, int host_rank, int iters, int buff_len,
                       const mpx_seq_opts* so, mpx_xfer_opts* o) {
    if (so->flags)
        return fail(MPX_ERR_INVALID, "flags %#x: a sequenced host-link call takes none (it reads no tx to stage)", so->flags);
    *o = mpx_xfer_opts{};
    o->check = so->check ? 1 : 0;
    o->timeout_ms = so->timeout_ms;
    o->nwg = so->nwg;
    TRY(check_hostlink(ctx, mode, group, gpu_rank, host_rank, iters, buff_len, o));
    const bool ack = mode == MPX_MODE_UNIDIR && group == 1;   // group: the caller's
    const u64 recv_len = ack ? 1 : (u64)buff_len;
    if (so->check && !so->expect && (u64)iters * recv_len > MPX_SEQ_AUTO_MAX)
        return fail(MPX_ERR_INVALID, "expect == NULL with %d x %llu B to generate on the CPU: above MPX_SEQ_AUTO_MAX (%llu)",
                    iters, recv_len, (u64)MPX_SEQ_AUTO_MAX);
    return MPX_OK;
}

// expect == NULL: the expectations on the CPU, before the timed part of the call
const uint64_t* seq_expectations(const mpx_seq_opts* so, u64 rx_key, int iters, u64 recv_len, std::vector<uint64_t>* own) {
    if (!so->check || so->expect) return so->expect;
    own->resize((size_t)(iters > 0 ? iters : 0));
    for (int i = 0; i < iters; ++i) (*own)[(size_t)i] = seq::expect(seq::key_of(rx_key, i), (size_t)recv_len);
    return own->data();
}

// the GPU side of a host-link call, ordinary (sq == nullptr) or sequenced;
// the arguments are checked
int gpu_hostlink(mpx_ctx* ctx, int mode, int my_group, int my_rank, int host_rank, int iters, void* tx, void* rx,
                 int buff_len, const mpx_xfer_opts* opts, const SeqCall* sq, double t_call, mpx_timing* t) {
    Rank& me = ctx->r[my_rank];
    const Rank& host = ctx->r[host_rank];
    if (!tx || !rx || tx != me.tx || rx != me.rx)
        return fail(MPX_ERR_INVALID, "tx/rx are not rank %d's attached buffers", my_rank);
    if (me.armed) return fail(MPX_ERR_STATE, "rank %d holds an armed call (start or disarm it first)", my_rank);
    if (me.broken) return fail(MPX_ERR_STATE, "rank %d: a previous transfer timed out", my_rank);
    const bool check = opts && opts->check;
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    if (check) TRY(ensure_csum(me, iters));

    const long long len = buff_len;
    const bool unidir = mode == MPX_MODE_UNIDIR;
    const long long send_len = (unidir && my_group == 0) ? 1 : len;
    const long long recv_len = (unidir && my_group == 1) ? 1 : len;
    hostlink::HostMailbox* hm = static_cast<hostlink::HostMailbox*>(host.host_mb_dev);
    XferArgs a{};
    a.tx = me.tx;
    a.rx = me.rx;
    a.peer_rx = host.host_rx_dev;
    a.peer_tx = host.host_tx_dev;
    a.my_mb = reinterpret_cast<Mailbox*>(&hm->out);     // what the endpoint writes and this rank polls
    a.peer_mb = reinterpret_cast<Mailbox*>(&hm->in);    // what this rank writes
    a.status = me.status;
    a.csum = me.csum;
    a.gbar = me.scratch;
    a.tx_seq0 = me.tx_seq[host_rank];
    a.rx_seq0 = me.rx_seq[host_rank];
    a.timeout_ticks = timeout_ticks(opts);
    a.len = len;
    a.iters = iters;
    a.mode = mode;
    a.group = my_group;
    a.my_slot = a.peer_slot = my_rank;   // the endpoint's rows are indexed by its GPU peer's rank
    a.nwg = hostlink_nwg(opts, len);
    a.check = check ? 1 : 0;
    a.ll_max = mpx_hostlink_ll_max();
    a.skip_push = test_knobs().skip_push;
    // the host-link recorder (mpx_hostlink_lat_enable): launch_hostlink then picks the traced kernels
    a.lat = (me.hostlink_lat.on && !sq) ? me.hostlink_lat.block(host_rank) : nullptr;
    // a sequenced call: k_hostlink_gen, never traced (the recorder's blocks stay as they are)
    if (sq) {
        a.seq = 1;
        a.seq_tx_key = sq->tx_key;
        a.seq_rx_key = sq->rx_key;
    }
    const bool ll_send = send_len <= a.ll_max, ll_recv = recv_len <= a.ll_max;
    const int grid = (ll_send && ll_recv) ? 1 : a.nwg;
    // bulk pushes read tx from LDS when one workgroup's chunk fits, as a pair's
    if (!sq && !(opts && (opts->flags & MPX_XFER_NOSTAGE)) && !ll_send && send_len > 0) {
        int per_block = 0;
        if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, me.dev) != hipSuccess) per_block = 0;
        const long long chunk = (((send_len + a.nwg - 1) / a.nwg) + 15) & ~15ll;
        if (chunk <= kStageMaxBytes && chunk <= (long long)per_block - 1024) a.stage = (int)chunk;
    }
    TRY(run_hostlink_kernel(me, my_rank, host_rank, a, grid, len <= a.ll_max, t_call, t));
    t->bytes = (uint64_t)buff_len * (uint64_t)iters * (unidir ? 1u : 2u);
    if (!check || iters <= 0) return MPX_OK;
    if (sq) return check_verdict(me, my_rank, 1, iters, (u64)recv_len, nullptr, t, nullptr, nullptr, sq->want);
    const bool ack = unidir && my_group == 1;
    const uint64_t want = ack ? opts->expect_ack : opts->expect_checksum;
    return check_verdict(me, my_rank, 1, iters, (u64)recv_len, &want, t, nullptr, nullptr);
}

// the endpoint's side, ordinary (sq == nullptr) or sequenced, on the calling
// thread; the arguments are checked
int host_side(mpx_ctx* ctx, int mode, int my_group, int host_rank, int peer_rank, int iters, int buff_len,
              const mpx_xfer_opts* opts, const SeqCall* sq, mpx_timing* t) {
    Rank& me = ctx->r[host_rank];
    if (me.broken) return fail(MPX_ERR_STATE, "host endpoint %d: a previous transfer timed out", host_rank);
    const TestKnobs knobs = test_knobs();
    hostlink::Call c;
    c.mb = static_cast<hostlink::HostMailbox*>(me.host_mb);
    c.tx = me.tx;
    c.rx = me.rx;
    c.gpu = peer_rank;
    c.mode = mode;
    c.group = my_group;
    c.iters = iters;
    c.len = buff_len;
    c.nwg = hostlink_nwg(opts, buff_len);
    c.ll_max = mpx_hostlink_ll_max();
    c.check = (opts && opts->check) ? 1 : 0;
    c.expect = opts ? opts->expect_checksum : 0;
    c.expect_ack = opts ? opts->expect_ack : 0;
    c.tx_seq0 = me.tx_seq[peer_rank];
    c.rx_seq0 = me.rx_seq[peer_rank];
    // the link's call number, as a GPU rank takes it (take_numbers): a call
    // that moves nothing posts nothing new
    if (iters > 0) ++me.calls[peer_rank];
    c.call = knobs.no_posted ? 0 : me.calls[peer_rank];
    c.timeout_s = (opts && opts->timeout_ms ? opts->timeout_ms : 10000) * 1e-3;
    c.skip_push = knobs.skip_push;
    c.lag_iter = knobs.host_lag_iter;
    c.lag_us = knobs.host_lag_us;
    if (sq) {
        c.seq_tx = me.tx;
        c.seq_tx_key = sq->tx_key;
        c.expect_each = sq->want;
        c.seq_stale = knobs.seq_stale;
    }
    // the endpoint's recorder (mpx_hostlink_lat_enable): the block of the GPU peer;
    // a sequenced call is never traced
    if (me.host_lat_on && !sq)
        c.lat = reinterpret_cast<hostlink::LatRec*>(me.host_lat + (size_t)peer_rank * hostlink::lat_rec_bytes(me.host_lat_cap));
    hostlink::Result r;
    const double t0 = now_s();
    const int rc = sq ? hostlink::run_seq(c, &r) : c.lat ? hostlink::run_loop<true>(c, &r) : hostlink::run(c, &r);
    t->wall_s = now_s() - t0;
    t->device_s = 0;
    t->launches = 0;
    t->nwg = buff_len <= c.ll_max ? 1 : c.nwg;
    t->protocol = buff_len <= c.ll_max ? kProtoHostLL : kProtoHostBulk;
    t->bytes = (uint64_t)buff_len * (uint64_t)iters * (mode == MPX_MODE_UNIDIR ? 1u : 2u);
    t->recv_done = r.recv_done;
    t->recv_digest = r.recv_digest;
    t->check_iters = r.check_iters;
    t->check_failures = r.check_failures;
    if (rc != 0) {
        me.broken = true;
        return fail(MPX_ERR_TIMEOUT, "host endpoint %d <- rank %d: a CPU wait timed out at iteration %d (mode %d, %d B)",
                    host_rank, peer_rank, r.where, mode, buff_len);
    }
    me.tx_seq[peer_rank] += (u64)iters;
    me.rx_seq[peer_rank] += (u64)iters;
    if (r.check_failures)
        return fail(MPX_ERR_CHECK, "host endpoint %d: %d of %llu received payloads failed the checksum", host_rank,
                    r.check_failures, (unsigned long long)r.check_iters);
    return MPX_OK;
}

}  // namespace

int mpx_xfer_hostlink(mpx_ctx* ctx, int mode, int my_group, int my_rank, int host_rank, int iters, void* tx, void* rx,
                      int buff_len, const mpx_xfer_opts* opts, mpx_timing* t) {
    if (!ctx || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    const double t_call = now_s();
    TRY(check_hostlink(ctx, mode, my_group, my_rank, host_rank, iters, buff_len, opts));
    return gpu_hostlink(ctx, mode, my_group, my_rank, host_rank, iters, tx, rx, buff_len, opts, nullptr, t_call, t);
}

int mpx_host_xfer(mpx_ctx* ctx, int mode, int my_group, int host_rank, int peer_rank, int iters, int buff_len,
                  const mpx_xfer_opts* opts, mpx_timing* t) {
    if (!ctx || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    TRY(check_hostlink(ctx, mode, my_group, peer_rank, host_rank, iters, buff_len, opts));
    return host_side(ctx, mode, my_group, host_rank, peer_rank, iters, buff_len, opts, nullptr, t);
}

// ---- sequenced payloads on the host link (include/mpx_hostlink_seq.h) -----------
// The ordinary call's two sides with the payload of iteration i generated
// from the link's key: k_hostlink_gen on the GPU, run_seq() on the endpoint.

int mpx_xfer_hostlink_seq(mpx_ctx* ctx, int mode, int my_group, int my_rank, int host_rank, int iters, void* tx, void* rx,
                          int buff_len, const mpx_seq_opts* opts, mpx_timing* t) {
    if (!ctx || !opts || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    const double t_call = now_s();
    mpx_xfer_opts o;
    TRY(check_hostlink_seq(ctx, mode, my_group, my_rank, host_rank, iters, buff_len, opts, &o));
    // (before the expectations are generated: every refusal comes before any work)
    const Rank& me = ctx->r[my_rank];
    if (!tx || !rx || tx != me.tx || rx != me.rx)
        return fail(MPX_ERR_INVALID, "tx/rx are not rank %d's attached buffers", my_rank);
    if (me.armed)
        return fail(MPX_ERR_STATE, "rank %d holds an armed call (a sequenced call cannot be armed: start or disarm it first)",
                    my_rank);
    if (me.broken) return fail(MPX_ERR_STATE, "rank %d: a previous transfer timed out", my_rank);
    const u64 recv_len = (mode == MPX_MODE_UNIDIR && my_group == 1) ? 1 : (u64)buff_len;
    SeqCall sq{seq::key_base(opts->seed, my_rank, host_rank), seq::key_base(opts->seed, host_rank, my_rank), nullptr};
    std::vector<uint64_t> own;
    sq.want = seq_expectations(opts, sq.rx_key, iters, recv_len, &own);
    return gpu_hostlink(ctx, mode, my_group, my_rank, host_rank, iters, tx, rx, buff_len, &o, &sq, t_call, t);
}

int mpx_host_xfer_seq(mpx_ctx* ctx, int mode, int my_group, int host_rank, int peer_rank, int iters, int buff_len,
                      const mpx_seq_opts* opts, mpx_timing* t) {
    if (!ctx || !opts || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    mpx_xfer_opts o;
    TRY(check_hostlink_seq(ctx, mode, my_group, peer_rank, host_rank, iters, buff_len, opts, &o));
    if (ctx->r[host_rank].broken) return fail(MPX_ERR_STATE, "host endpoint %d: a previous transfer timed out", host_rank);
    const u64 recv_len = (mode == MPX_MODE_UNIDIR && my_group == 1) ? 1 : (u64)buff_len;
    SeqCall sq{seq::key_base(opts->seed, host_rank, peer_rank), seq::key_base(opts->seed, peer_rank, host_rank), nullptr};
    std::vector<uint64_t> own;
    sq.want = seq_expectations(opts, sq.rx_key, iters, recv_len, &own);
    return host_side(ctx, mode, my_group, host_rank, peer_rank, iters, buff_len, &o, &sq, t);
}

// ---- the host-link recorder (include/mpx_hostlink_lat.h) -----------------------
// A GPU rank's blocks are a third Recorder (Rank.hostlink_lat: device memory,
// mpx_runtime.hip's helpers); an endpoint's are hostlink::LatRec blocks in
// ordinary host memory, read and cleared right here.

namespace {
static_assert(sizeof(hostlink::LatRec) == sizeof(LatBlock) && offsetof(hostlink::LatRec, hist) == offsetof(LatBlock, hist) &&
                  offsetof(hostlink::LatRec, raw) == offsetof(LatBlock, raw),
              "LatRec has the device block's layout");

hostlink::LatRec* host_lat_block(const Rank& h, int i) {
    return reinterpret_cast<hostlink::LatRec*>(h.host_lat + (size_t)i * hostlink::lat_rec_bytes(h.host_lat_cap));
}
void host_lat_clear(Rank& h, int blocks) {
    for (int i = 0; i < blocks; ++i) {
        hostlink::LatRec* b = host_lat_block(h, i);
        memset(b, 0, offsetof(hostlink::LatRec, raw));
        b->raw_cap = (uint64_t)h.host_lat_cap;
    }
}
// The rank a host-link recorder call names: 1 = an attached local GPU rank
// (holding no armed call), 2 = a host endpoint; else the status in *rc.
int hostlink_lat_rank(mpx_ctx* ctx, int rank, int* rc) {
    *rc = MPX_OK;
    if (!ctx) {
        *rc = fail(MPX_ERR_INVALID, "ctx is NULL");
        return 0;
    }
    if (rank >= 0 && rank < ctx->nranks && ctx->r[rank].host) return 2;
    if (rank < 0 || rank >= ctx->nranks || !ctx->r[rank].local) {
        *rc = fail(MPX_ERR_INVALID, "rank %d is neither a local GPU rank nor a host endpoint", rank);
        return 0;
    }
    if (ctx->r[rank].armed) {
        *rc = fail(MPX_ERR_STATE, "rank %d holds an armed call (start or disarm it first)", rank);
        return 0;
    }
    return 1;
}
int hostlink_lat_peer(const mpx_ctx* ctx, int rank, int peer) {
    if (peer < 0 || peer >= ctx->nranks || peer == rank) return fail(MPX_ERR_INVALID, "rank %d: peer rank %d", rank, peer);
    return MPX_OK;
}
int hostlink_lat_off(int rank) { return fail(MPX_ERR_STATE, "rank %d: the host-link recorder is not enabled", rank); }
}  // namespace

int mpx_hostlink_lat_enable(mpx_ctx* ctx, int rank, int raw_cap) {
    if (!ctx) return fail(MPX_ERR_INVALID, "ctx is NULL");
    if (ctx->engine != MPX_ENGINE_KERNEL)
        return fail(MPX_ERR_UNSUPPORTED, "the host-link recorder runs inside the kernel engine's host-link loop: not this engine");
    int rc;
    const int kind = hostlink_lat_rank(ctx, rank, &rc);
    if (!kind) return rc;
    Rank& me = ctx->r[rank];
    if (kind == 1) return recorder_enable(me, me.hostlink_lat, ctx->nranks, raw_cap, MPX_HOSTLINK_LAT_RAW_MAX, "host-link recorder");
    if (raw_cap < 0 || raw_cap > MPX_HOSTLINK_LAT_RAW_MAX)
        return fail(MPX_ERR_INVALID, "raw_cap %d not in [0,%d]", raw_cap, MPX_HOSTLINK_LAT_RAW_MAX);
    if (!me.host_lat || me.host_lat_alloc < raw_cap) {
        const size_t bytes = (size_t)ctx->nranks * hostlink::lat_rec_bytes(raw_cap);
        void* p = malloc(bytes);
        if (!p) return fail(MPX_ERR_NOMEM, "host-link recorder of %zu B", bytes);
        free(me.host_lat);
        me.host_lat = static_cast<unsigned char*>(p);
        me.host_lat_alloc = raw_cap;
    }
    me.host_lat_cap = raw_cap;
    host_lat_clear(me, ctx->nranks);
    me.host_lat_on = true;
    return MPX_OK;
}

int mpx_hostlink_lat_disable(mpx_ctx* ctx, int rank) {
    int rc;
    const int kind = hostlink_lat_rank(ctx, rank, &rc);
    if (!kind) return rc;
    if (kind == 1) ctx->r[rank].hostlink_lat.on = false;   // the blocks stay until finalize
    else ctx->r[rank].host_lat_on = false;
    return MPX_OK;
}

int mpx_hostlink_lat_reset(mpx_ctx* ctx, int rank) {
    int rc;
    const int kind = hostlink_lat_rank(ctx, rank, &rc);
    if (!kind) return rc;
    Rank& me = ctx->r[rank];
    if (kind == 1) return me.hostlink_lat.on ? recorder_reset(me, me.hostlink_lat) : hostlink_lat_off(rank);
    if (!me.host_lat_on) return hostlink_lat_off(rank);
    host_lat_clear(me, ctx->nranks);
    return MPX_OK;
}

int mpx_hostlink_lat_get(mpx_ctx* ctx, int rank, int peer, mpx_lat* out) {
    int rc;
    const int kind = hostlink_lat_rank(ctx, rank, &rc);
    if (!kind) return rc;
    if (!out) return fail(MPX_ERR_INVALID, "NULL argument");
    TRY(hostlink_lat_peer(ctx, rank, peer));
    Rank& me = ctx->r[rank];
    if (kind == 1) return me.hostlink_lat.on ? recorder_get(me, me.hostlink_lat, peer, out) : hostlink_lat_off(rank);
    if (!me.host_lat_on) return hostlink_lat_off(rank);
    const hostlink::LatRec& b = *host_lat_block(me, peer);
    memset(out, 0, sizeof *out);
    out->count = b.count;
    out->calls = b.calls;
    out->min_ticks = b.min_ticks;
    out->max_ticks = b.max_ticks;
    out->sum_ticks = b.sum_ticks;
    out->max_iter = b.max_iter;
    out->last_iters = b.last_iters;
    out->tick_s = 1e-9;   // CLOCK_MONOTONIC in nanoseconds
    static_assert(sizeof out->hist == sizeof b.hist, "mpx_lat and LatRec histograms differ");
    memcpy(out->hist, b.hist, sizeof b.hist);
    return MPX_OK;
}

int mpx_hostlink_lat_raw(mpx_ctx* ctx, int rank, int peer, uint64_t* stamps, int cap, int* n) {
    int rc;
    const int kind = hostlink_lat_rank(ctx, rank, &rc);
    if (!kind) return rc;
    if (!n || cap < 0 || (!stamps && cap > 0)) return fail(MPX_ERR_INVALID, "bad argument");
    *n = 0;
    TRY(hostlink_lat_peer(ctx, rank, peer));
    Rank& me = ctx->r[rank];
    if (kind == 1) return me.hostlink_lat.on ? recorder_raw(me, me.hostlink_lat, peer, stamps, cap, n) : hostlink_lat_off(rank);
    if (!me.host_lat_on) return hostlink_lat_off(rank);
    const hostlink::LatRec& b = *host_lat_block(me, peer);
    // t[0] alone says nothing: with raw_cap = 0 no stamp is reported (as a GPU rank's)
    uint64_t have = me.host_lat_cap > 0 ? b.raw_n : 0;
    if (have > (uint64_t)me.host_lat_cap + 1) have = (uint64_t)me.host_lat_cap + 1;
    if (have > (uint64_t)cap) have = (uint64_t)cap;
    if (have) memcpy(stamps, b.raw, (size_t)have * sizeof(uint64_t));
    *n = (int)have;
    return MPX_OK;
}

// ---- the full-duplex loop (include/mpx_hostlink_duplex.h) ----------------------

namespace {
// check_hostlink's rules (there is no mode and no group), and a per-direction
// width whose split grid fits
int check_duplex(mpx_ctx* ctx, int gpu_rank, int host_rank, int iters, int buff_len, const mpx_xfer_opts* o) {
    TRY(check_hostlink(ctx, MPX_MODE_PINGPONG, 0, gpu_rank, host_rank, iters, buff_len, o));
    const int nwg = hostlink_nwg(o, buff_len);
    if (nwg > kDuplexMaxWG)
        return fail(MPX_ERR_INVALID, "nwg %d per direction: the split grid would exceed %d workgroups", nwg, kMaxPushWG);
    return MPX_OK;
}
}  // namespace

int mpx_xfer_hostlink_duplex(mpx_ctx* ctx, int my_rank, int host_rank, int iters, void* tx, void* rx, int buff_len,
                             const mpx_xfer_opts* opts, mpx_timing* t) {
    if (!ctx || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    const double t_call = now_s();
    TRY(check_duplex(ctx, my_rank, host_rank, iters, buff_len, opts));
    Rank& me = ctx->r[my_rank];
    const Rank& host = ctx->r[host_rank];
    if (!tx || !rx || tx != me.tx || rx != me.rx)
        return fail(MPX_ERR_INVALID, "tx/rx are not rank %d's attached buffers", my_rank);
    if (me.armed) return fail(MPX_ERR_STATE, "rank %d holds an armed call (start or disarm it first)", my_rank);
    if (me.broken) return fail(MPX_ERR_STATE, "rank %d: a previous transfer timed out", my_rank);
    const bool check = opts && opts->check;
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    if (check) TRY(ensure_csum(me, iters));

    const long long len = buff_len;
    hostlink::HostMailbox* hm = static_cast<hostlink::HostMailbox*>(host.host_mb_dev);
    XferArgs a{};
    a.tx = me.tx;
    a.rx = me.rx;
    a.peer_rx = host.host_rx_dev;
    a.peer_tx = host.host_tx_dev;
    a.my_mb = reinterpret_cast<Mailbox*>(&hm->out);
    a.peer_mb = reinterpret_cast<Mailbox*>(&hm->in);
    a.status = me.status;
    a.csum = me.csum;
    a.gbar = me.scratch;
    a.tx_seq0 = me.tx_seq[host_rank];
    a.rx_seq0 = me.rx_seq[host_rank];
    a.timeout_ticks = timeout_ticks(opts);
    a.len = len;
    a.iters = iters;
    a.mode = MPX_MODE_NONBLOCKING;
    a.my_slot = a.peer_slot = my_rank;
    a.nwg = hostlink_nwg(opts, len);   // per direction
    a.check = check ? 1 : 0;
    a.nb_publish = nb_publish();
    a.skip_push = test_knobs().skip_push;
    if (!(opts && (opts->flags & MPX_XFER_NOSTAGE)) && len > 0) {
        int per_block = 0;
        if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, me.dev) != hipSuccess) per_block = 0;
        const long long chunk = (((len + a.nwg - 1) / a.nwg) + 15) & ~15ll;
        if (chunk <= kStageMaxBytes && chunk <= (long long)per_block - 1024) a.stage = (int)chunk;
    }
    TRY(run_hostlink_duplex_kernel(me, my_rank, host_rank, a, t_call, t));
    t->bytes = 2ull * (uint64_t)buff_len * (uint64_t)iters;
    if (!check || iters <= 0) return MPX_OK;
    const uint64_t want = opts->expect_checksum;
    return check_verdict(me, my_rank, 1, iters, (u64)len, &want, t, nullptr, nullptr);
}

int mpx_host_xfer_duplex(mpx_ctx* ctx, int host_rank, int peer_rank, int iters, int buff_len, const mpx_xfer_opts* opts,
                         mpx_timing* t) {
    if (!ctx || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    TRY(check_duplex(ctx, peer_rank, host_rank, iters, buff_len, opts));
    Rank& me = ctx->r[host_rank];
    if (me.broken) return fail(MPX_ERR_STATE, "host endpoint %d: a previous transfer timed out", host_rank);
    const TestKnobs knobs = test_knobs();
    hostlink::Call c;
    c.mb = static_cast<hostlink::HostMailbox*>(me.host_mb);
    c.tx = me.tx;
    c.rx = me.rx;
    c.gpu = peer_rank;
    c.mode = MPX_MODE_NONBLOCKING;
    c.iters = iters;
    c.len = buff_len;
    c.nwg = hostlink_nwg(opts, buff_len);
    c.check = (opts && opts->check) ? 1 : 0;
    c.expect = opts ? opts->expect_checksum : 0;
    c.tx_seq0 = me.tx_seq[peer_rank];
    c.rx_seq0 = me.rx_seq[peer_rank];
    if (iters > 0) ++me.calls[peer_rank];   // (as mpx_host_xfer)
    c.call = knobs.no_posted ? 0 : me.calls[peer_rank];
    c.timeout_s = (opts && opts->timeout_ms ? opts->timeout_ms : 10000) * 1e-3;
    hostlink::Result r;
    const double t0 = now_s();
    const int rc = hostlink::run_duplex(c, &r);
    t->wall_s = now_s() - t0;
    t->device_s = 0;
    t->launches = 0;
    t->nwg = c.nwg;
    t->protocol = kProtoHostDuplex;
    t->bytes = 2ull * (uint64_t)buff_len * (uint64_t)iters;
    t->recv_done = r.recv_done;
    t->recv_digest = r.recv_digest;
    t->check_iters = r.check_iters;
    t->check_failures = r.check_failures;
    if (rc != 0) {
        me.broken = true;
        return fail(MPX_ERR_TIMEOUT, "host endpoint %d <- rank %d: a CPU wait timed out at iteration %d (full duplex, %d B)",
                    host_rank, peer_rank, r.where, buff_len);
    }
    me.tx_seq[peer_rank] += (u64)iters;
    me.rx_seq[peer_rank] += (u64)iters;
    if (r.check_failures)
        return fail(MPX_ERR_CHECK, "host endpoint %d: %d of %llu received payloads failed the checksum", host_rank,
                    r.check_failures, (unsigned long long)r.check_iters);
    return MPX_OK;
}

}  // extern "C"
