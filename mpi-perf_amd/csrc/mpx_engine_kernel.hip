// mpx_engine_kernel.hip — the kernel engine's host side: one lifecycle (take
// the call's numbers, launch, complete) that the pair call (run_kernel), the
// armed call (mpx_xfer_arm, start_armed, disarm), the fan call (mpx_xfer_fan)
// and the host-link call (run_hostlink_kernel) all go through.
#include "mpx_runtime.h"
#include "mpx_seq.h"

#include <algorithm>

using namespace mpx;

namespace mpx {
namespace {

// How a kernel-engine call waits for its kernel (MPX_SYNC, read once):
//   query (default) — spin on the host-mapped completion word the kernel's
//           last workgroup stores (Status.done), then on hipEventQuery of the
//           end event: the call returns once the kernel has retired (its
//           writes visible to every later command), with no interrupt on
//           the way;
//   event — hipEventSynchronize (round 3's form: the runtime's blocking
//           wait, woken by an interrupt once its short active spin expires).
// run-hbv3's 456131 B x 10 calls carried ~21 us of fixed
// cost each; mpx_last_phases reports where a call's time goes.
enum SyncMode { kSyncQuery = 0, kSyncEvent = 1 };
int sync_mode() {
    static const int m = [] {
        const char* v = getenv("MPX_SYNC");
        return (v && !strcmp(v, "event")) ? kSyncEvent : kSyncQuery;
    }();
    return m;
}

inline void cpu_relax() { __builtin_ia32_pause(); }

// What every kernel-engine call — pair, armed or fan — carries through its
// lifecycle: take_numbers, launch_call, complete_call.
struct Call {
    int my_rank = 0, iters = 0;
    // the numbers the call took: the rank's token, and the peers whose
    // calls[] it incremented — one for a pair, npeers for a fan, none when
    // iters == 0 (a call that moves nothing posts nothing new: the count
    // stays equal on both sides even if only one side makes such a call)
    u64 token = 0;
    int npeers = 0;
    int peer[MPX_MAX_RANKS];
    bool launched = false;           // the kernel was enqueued: the numbers are spent
    // launch
    bool fail_launch = false;        // MPX_TEST fail_launch names this rank: fail before the enqueue
    size_t csum_words = 0;           // checksum words zeroed ahead of the kernel (check mode)
    size_t cnt_words = 0;            //   and checked-chunk counters (non-blocking check mode)
    const FanTable* table = nullptr; // fan: the link table's host image, copied to the device first
    bool armed = false;              // launched ahead of the call: no events, starts at the go store
    bool resident = false;           // armed: every workgroup was waiting when arm returned
    double t0 = 0;                   // the start of the timed call: just before the start event
                                     // (pair) or the table copy (fan), or the go store (armed)
    // completion
    int nwg = 0, protocol = 0;       // reported in mpx_timing
    const char* kernel = "";         // the kernel's name in the caller's error texts
};

// Takes the call's numbers: the rank's token, and — when iters > 0 — the next
// call number on the link to each peer.  call[k] is what the kernel posts and
// awaits on link k (Mailbox.posted); the no_posted knob zeroes it (every wait
// for posted >= 0 holds at once) and leaves the count alone.
void take_numbers(Rank& me, Call& c, const int* peers, int npeers, bool no_posted, u64* call) {
    c.token = ++me.token;
    c.npeers = 0;
    for (int k = 0; k < npeers; ++k) {
        if (c.iters > 0) ++me.calls[c.peer[c.npeers++] = peers[k]];
        call[k] = no_posted ? 0 : me.calls[peers[k]];
    }
}

// A call that failed before its kernel was enqueued gives back what it took
// (its token and the links' call numbers): the peers never see those numbers,
// and a later call must post the ones they wait for.  Once the
// kernel is enqueued the numbers stay taken — the kernel posts them — whatever
// fails after it; except `cancelled`, an armed call ended without a transfer
// (disarm): its kernel consumed the token and exited before posting its
// receives, so the call numbers alone come back.
void give_back(Rank& me, const Call& c, bool cancelled = false) {
    if (c.launched && !cancelled) return;
    for (int k = 0; k < c.npeers; ++k) --me.calls[c.peer[k]];
    if (!c.launched) --me.token;
}

}  // namespace

// One pair call: its arguments and launch shape, built by prepare_call;
// launched at once (run_kernel) or armed ahead of the host's barrier
// (mpx_xfer_arm) and started later (start_armed).
struct KernelCall {
    XferArgs a{};
    Call c;
    int grid = 0;
    int peer_rank = 0, mode = 0, group = 0;
    long long len = 0;
    // what an armed call was armed with: mpx_xfer_ex must match it
    int check = 0, flags = 0, nwg_opt = 0;
    uint32_t timeout_ms = 0;
    uint64_t expect = 0, expect_ack = 0;
};

namespace {

// Wait for the call's completion.  Unarmed: the end event ev1 (see
// sync_mode); *t_done = when the completion word was first seen (0 in event
// mode).  Armed: the completion word only — every byte the kernel leaves for
// the host or another stream (rx included: LL unpacks are write-through) is
// in memory before it is stored; the stream is polled every 50 us so that a
// kernel that ended without storing it (it cannot, but a fault could) ends
// the wait with an error instead of a hang.
// The call's end line (Status.fin) is complete and sealed for `token`: its
// word carries the token and the seal of the other seven words as read now
// (a line seen half-written does not match; the caller reads it again).
bool fin_sealed(const Rank& me, u64 token, Fin* out) {
    const volatile Fin* f = &me.status->fin;
    const u64 w = __atomic_load_n(&me.status->fin.word, __ATOMIC_ACQUIRE);
    if ((w & 0xffffffffull) != (token & 0xffffffffull)) return false;
    Fin v;
    v.recv_done = f->recv_done;
    v.recv_digest = f->recv_digest;
    v.t_entry = f->t_entry;
    v.t_posted = f->t_posted;
    v.t_first = f->t_first;
    v.t_loop = f->t_loop;
    v.t_exit = f->t_exit;
    v.word = w;
    if (fin_word(token, v.recv_done, v.recv_digest, v.t_entry, v.t_posted, v.t_first, v.t_loop, v.t_exit) != w)
        return false;
    if (out) *out = v;
    return true;
}

int wait_kernel(Rank& me, u64 token, bool armed, double* t_done) {
    *t_done = 0;
    if (!armed && sync_mode() == kSyncEvent) {
        HIPCK(hipEventSynchronize(me.ev1));
        return MPX_OK;
    }
    // Before the word arrives the end event / stream is polled only every
    // 50 us (a kernel that could not launch never stores it); after, back to
    // back (unarmed) or not at all (armed).
    double next_query = now_s() + 50e-6;
    for (;;) {
        if (*t_done == 0 && fin_sealed(me, token, nullptr)) {
            *t_done = now_s();
            if (armed) return MPX_OK;
        }
        if (*t_done != 0 || now_s() >= next_query) {
            const hipError_t q = armed ? hipStreamQuery(me.stream) : hipEventQuery(me.ev1);
            if (q == hipSuccess) {
                if (armed && !fin_sealed(me, token, nullptr))
                    return fail(MPX_ERR_HIP, "armed transfer kernel ended without its completion line");
                if (*t_done == 0) *t_done = now_s();
                return MPX_OK;
            }
            if (q != hipErrorNotReady) HIPCK(q);
            next_query = now_s() + 50e-6;
        }
        cpu_relax();
    }
}

int prepare_call(mpx_ctx* ctx, Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters,
                 long long len, const mpx_xfer_opts* o, KernelCall* kc) {
    XferArgs& a = kc->a;
    a = XferArgs{};
    a.tx = me.tx;
    a.rx = me.rx;
    a.peer_rx = peer.rx;
    a.my_mb = me.mb;
    a.peer_mb = peer.mb;
    a.status = me.status;
    a.csum = me.csum;
    a.gbar = me.scratch;
    a.tx_seq0 = me.tx_seq[peer_rank];
    a.rx_seq0 = me.rx_seq[peer_rank];
    a.timeout_ticks = timeout_ticks(o);
    a.len = len;
    a.iters = iters;
    a.mode = mode;
    a.group = group;
    a.my_slot = my_rank;
    a.peer_slot = peer_rank;
    // push workgroups: the call's option, else MPX_PUSH_WG (every rank of a
    // job inherits the same environment, so both sides agree), else the
    // size rule bulk_nwg(); narrowed for small pushes (link_nwg)
    static const int env_nwg = [] {
        const char* v = getenv("MPX_PUSH_WG");
        return v ? atoi(v) : 0;
    }();
    const int opt_nwg = (o && o->nwg > 0) ? o->nwg : 0;
    a.nwg = link_nwg(opt_nwg, env_nwg, bulk_nwg(len, same_device(me, peer)), len);
    if (a.nwg < 1) return fail(MPX_ERR_INVALID, "nwg %d > %d", opt_nwg ? opt_nwg : env_nwg, kMaxPushWG);
    a.check = (o && o->check) ? 1 : 0;
    static const bool env_stream = [] {
        const char* v = getenv("MPX_PUSH_STREAM");
        return v && atoi(v) != 0;
    }();
    a.stream = ((o && (o->flags & MPX_XFER_STREAM)) || env_stream) ? 1 : 0;
    a.nb_publish = nb_publish();
    a.ll_max = ll_max_bytes(same_device(me, peer));
    if (const char* v = getenv("MPX_LL_MAX")) a.ll_max = atoi(v) < kLLMaxBytes ? atoi(v) : kLLMaxBytes;
    a.cnt = me.cnt;
    // the latency recorder traces the blocking loops only (launch_xfer)
    a.lat = (me.lat.on && mode != MPX_MODE_NONBLOCKING) ? me.lat.block(0) : nullptr;
    const TestKnobs knobs = test_knobs();
    a.skip_push = knobs.skip_push;
    a.no_pull_wait = knobs.no_pull_wait ? 1 : 0;
    if (knobs.lag_rank == my_rank && knobs.lag_us > 0) {
        a.lag_wg = knobs.lag_wg;
        a.lag_ticks = (u64)knobs.lag_us * 100ull;   // s_memrealtime: 100 MHz
    }
    if (a.lag_wg < 0) a.lag_wg += a.nwg;   // -1: the last pushing workgroup

    const bool ll = mode != MPX_MODE_NONBLOCKING && len <= a.ll_max;
    const bool pushes_len = mode != MPX_MODE_UNIDIR || group == 1;
    const bool recvs_len = mode != MPX_MODE_UNIDIR || group == 0;
    // pull mode: B-byte payloads are loaded by their receiver (k_xfer_pull);
    // LL messages stay pushes.  A receiving side runs nwg workgroups (one
    // chunk each), unidir group 1 one (it only publishes and takes acks).
    a.pull = (!ll && pull_requested(o)) ? 1 : 0;
    {
        // fields another rank's thread may set at the same time (a lazily
        // mapped tx, a lazily allocated ring) are read under the context lock
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (a.pull) TRY(ensure_peer_tx_locked(ctx, peer, peer_rank));
        a.peer_tx = peer.tx;
        a.ring = me.ring;
        a.peer_ring = peer.ring;
        a.slots = link_slots(me, peer, len);
    }
    if (!a.pull && a.check && mode == MPX_MODE_NONBLOCKING && len > 0 && a.slots > 1 && (!a.ring || !a.peer_ring))
        return fail(MPX_ERR_STATE, "rank %d/%d: check-mode receive ring missing", my_rank, peer_rank);
    kc->grid = a.pull ? (recvs_len ? a.nwg : 1) : (!ll && (pushes_len || (a.check && recvs_len))) ? a.nwg : 1;
    // bulk pushes read tx from LDS when one workgroup's chunk fits
    // (kStageMaxBytes); the call's MPX_XFER_NOSTAGE flag reads it from HBM
    if (!(o && (o->flags & MPX_XFER_NOSTAGE)) && !ll && !a.pull && pushes_len && len > 0) {
        static const long long lds_cap = [] {
            int dev = 0, per_block = 0;
            (void)hipGetDevice(&dev);
            if (hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess)
                per_block = 0;
            return (long long)per_block - 1024;   // room for k_xfer's static LDS
        }();
        const long long chunk = (((len + a.nwg - 1) / a.nwg) + 15) & ~15ll;
        if (chunk <= kStageMaxBytes && chunk <= lds_cap) a.stage = (int)chunk;
    }
    Call& c = kc->c;
    c.my_rank = my_rank;
    c.iters = iters;
    c.kernel = "transfer kernel";
    c.fail_launch = knobs.fail_launch == my_rank;
    c.nwg = ll ? 1 : a.nwg;
    c.protocol = ll ? kProtoLL : a.pull ? kProtoPull : kProtoBulk;
    if (a.check) {
        c.csum_words = (size_t)iters;
        if (mode == MPX_MODE_NONBLOCKING) c.cnt_words = (size_t)iters;
    }
    take_numbers(me, c, &peer_rank, 1, knobs.no_posted, &a.call);
    a.done_token = c.token;
    kc->peer_rank = peer_rank;
    kc->mode = mode;
    kc->group = group;
    kc->len = len;
    kc->check = a.check;
    kc->flags = o ? o->flags : 0;
    kc->nwg_opt = o ? o->nwg : 0;
    kc->timeout_ms = o ? o->timeout_ms : 0;
    kc->expect = o ? o->expect_checksum : 0;
    kc->expect_ack = o ? o->expect_ack : 0;
    return MPX_OK;
}

// Enqueue the call's kernel on the rank's stream with `enqueue` (launch_xfer
// or launch_fan; scratch words [0..3] and [8] are zero: the previous call's
// last workgroup reset them — no memset ahead of the kernel).  Armed: no
// events (the kernel's span comes from its own clock).
template <class Enqueue>
int launch_call(Rank& me, Call& c, Enqueue enqueue) {
    if (c.fail_launch)
        return fail(MPX_ERR_HIP, "rank %d: launch failed (MPX_TEST fail_launch)", c.my_rank);
    c.t0 = 0;
    if (c.table) {
        memcpy(me.fan_host, c.table, sizeof(FanTable));
        c.t0 = now_s();
        HIPCK(hipMemcpyAsync(me.fan_tab, me.fan_host, sizeof(FanTable), hipMemcpyHostToDevice, me.stream));
    }
    if (c.csum_words) HIPCK(hipMemsetAsync(me.csum, 0, c.csum_words * sizeof(u64), me.stream));
    if (c.cnt_words) HIPCK(hipMemsetAsync(me.cnt, 0, c.cnt_words * sizeof(u64), me.stream));
    me.status->err = 0;
    me.status->where = 0;
    memset(&me.status->fin, 0, sizeof(Fin));
    if (c.t0 == 0) c.t0 = now_s();
    if (!c.armed) HIPCK(hipEventRecord(me.ev0, me.stream));
    HIPCK(enqueue());
    c.launched = true;
    if (!c.armed) HIPCK(hipEventRecord(me.ev1, me.stream));
    return MPX_OK;
}

// Wait for the call, then its timing, phases and receive accounting; the
// links to `peers` advance by the call's iterations.  c.t0 = the start of the
// timed call.  timed_out(iteration) reports the caller's device-wait timeout.
template <class TimedOut>
int complete_call(Rank& me, const Call& c, const int* peers, int npeers, double t_call, mpx_timing* t, Fin* fin_out,
                  TimedOut timed_out) {
    double t_done = 0;
    TRY(wait_kernel(me, c.token, c.armed, &t_done));
    const double t_end = now_s();
    t->wall_s = t_end - c.t0;
    // the end line: sealed once wait_kernel returns (a retired kernel wrote
    // it whole); a line that does not match here is a kernel that never
    // wrote it (a fault) and fails the call
    Fin fin{};
    if (!fin_sealed(me, c.token, &fin))
        return fail(MPX_ERR_HIP, "rank %d: the %s left no completion line", c.my_rank, c.kernel);
    if (fin_out) *fin_out = fin;
    const u64 te = fin.t_entry, tp = fin.t_posted, tx = fin.t_exit;
    const double kernel_s = (te && tx >= te) ? (double)(tx - te) * 1e-8 : 0;
    if (c.armed) {
        t->device_s = kernel_s;   // from go seen to the last workgroup's end (s_memrealtime)
    } else {
        float ms = 0;
        HIPCK(hipEventElapsedTime(&ms, me.ev0, me.ev1));
        t->device_s = ms * 1e-3;
    }
    t->launches = 1;
    t->nwg = c.nwg;
    t->protocol = c.protocol;
    t->recv_done = fin.recv_done;
    t->recv_digest = fin.recv_digest;
    // phases (mpx_last_phases): the kernel's own clock splits its span; the
    // host's clock brackets it (launch or go before, completion after)
    mpx_phases& ph = me.phases;
    ph = mpx_phases{};
    ph.wall_s = t->wall_s;
    ph.host_prep_s = c.armed ? 0 : c.t0 - t_call;
    ph.kernel_s = kernel_s;
    ph.posted_wait_s = (te && tp >= te) ? (double)(tp - te) * 1e-8 : 0;
    if (t_done > 0 && kernel_s > 0) {
        ph.launch_to_start_s = (t_done - c.t0) - kernel_s;
        ph.done_to_return_s = t_end - t_done;
    }
    ph.armed = c.armed ? 1 : 0;
    ph.resident = (c.armed && c.resident) ? 1 : 0;
    // inside the kernel: the first iteration from the moment this side could
    // start it (k_xfer; k_xfer_fan never stamps t_first, so it reads 0), and
    // the end after the loop
    const u64 tf = fin.t_first, tl = fin.t_loop;
    const u64 t_go = tp >= te ? tp : te;
    ph.first_iter_s = (te && tf >= t_go) ? (double)(tf - t_go) * 1e-8 : 0;
    ph.tail_s = (tl && tx >= tl) ? (double)(tx - tl) * 1e-8 : 0;
    const unsigned err = __atomic_load_n(&me.status->err, __ATOMIC_ACQUIRE);
    if (err == 2) {
        me.broken = true;
        return fail(MPX_ERR_TIMEOUT, "rank %d: the armed transfer was not started within its deadline", c.my_rank);
    }
    if (err) {
        me.broken = true;
        return timed_out(me.status->where - 1);
    }
    for (int k = 0; k < npeers; ++k) {
        me.tx_seq[peers[k]] += (u64)c.iters;
        me.rx_seq[peers[k]] += (u64)c.iters;
    }
    return MPX_OK;
}

int complete_pair(Rank& me, const KernelCall& kc, double t_call, mpx_timing* t) {
    return complete_call(me, kc.c, &kc.peer_rank, 1, t_call, t, nullptr, [&](unsigned iteration) {
        return fail(MPX_ERR_TIMEOUT, "rank %d <- rank %d: device wait timed out at iteration %u (mode %d, %lld B)",
                    kc.c.my_rank, kc.peer_rank, iteration, kc.mode, kc.len);
    });
}

// does an armed call match the arguments mpx_xfer_ex was given?
bool armed_matches(const KernelCall& kc, int mode, int group, int peer_rank, int iters, long long len,
                   const mpx_xfer_opts* o) {
    return kc.mode == mode && kc.group == group && kc.peer_rank == peer_rank && kc.c.iters == iters && kc.len == len &&
           kc.check == ((o && o->check) ? 1 : 0) && kc.flags == (o ? o->flags : 0) && kc.nwg_opt == (o ? o->nwg : 0) &&
           kc.timeout_ms == (o ? o->timeout_ms : 0) && kc.expect == (o ? o->expect_checksum : 0) &&
           kc.expect_ack == (o ? o->expect_ack : 0);
}

}  // namespace

int run_kernel(mpx_ctx* ctx, Rank& me, Rank& peer, int my_rank, int peer_rank, int mode, int group, int iters,
               long long len, const mpx_xfer_opts* o, mpx_timing* t, const u64* seq_keys) {
    const double t_call = now_s();
    KernelCall kc;
    TRY(prepare_call(ctx, me, peer, my_rank, peer_rank, mode, group, iters, len, o, &kc));
    if (seq_keys) {
        // a sequenced call: the same arguments and launch shape; the pushes
        // are generated, so there is no tx to stage, and it is never traced
        kc.a.seq = 1;
        kc.a.seq_tx_key = seq_keys[0];
        kc.a.seq_rx_key = seq_keys[1];
        kc.a.stage = 0;
        kc.a.lat = nullptr;
    }
    const int st = launch_call(me, kc.c, [&] { return launch_xfer(kc.a, kc.grid, me.stream); });
    if (st != MPX_OK) {
        give_back(me, kc.c);
        return st;
    }
    return complete_pair(me, kc, t_call, t);
}

// A host-link call (mpx_xfer_hostlink, mpx_xfer_hostlink_duplex; its arguments
// are built in mpx_engine_hostlink.hip): the same three steps with the host
// link's kernel, which `enqueue` launches.
namespace {
template <class Enqueue>
int run_hostlink_call(Rank& me, int my_rank, int host_rank, XferArgs& a, int nwg, int protocol, double t_call,
                      mpx_timing* t, Enqueue enqueue) {
    const TestKnobs knobs = test_knobs();
    Call c;
    c.my_rank = my_rank;
    c.iters = a.iters;
    c.kernel = "host-link kernel";
    c.fail_launch = knobs.fail_launch == my_rank;
    c.nwg = nwg;
    c.protocol = protocol;
    if (a.check) c.csum_words = (size_t)a.iters;
    take_numbers(me, c, &host_rank, 1, knobs.no_posted, &a.call);
    a.done_token = c.token;
    const int st = launch_call(me, c, enqueue);
    if (st != MPX_OK) {
        give_back(me, c);
        return st;
    }
    return complete_call(me, c, &host_rank, 1, t_call, t, nullptr, [&](unsigned iteration) {
        return fail(MPX_ERR_TIMEOUT, "rank %d <- host endpoint %d: device wait timed out at iteration %u (mode %d, %lld B)",
                    my_rank, host_rank, iteration, a.mode, a.len);
    });
}
}  // namespace

int run_hostlink_kernel(Rank& me, int my_rank, int host_rank, XferArgs& a, int grid, bool ll, double t_call,
                        mpx_timing* t) {
    return run_hostlink_call(me, my_rank, host_rank, a, ll ? 1 : a.nwg, ll ? kProtoHostLL : kProtoHostBulk, t_call, t,
                             [&] { return launch_hostlink(a, grid, me.stream); });
}

// the full-duplex loop (k_hostlink_duplex): a.nwg is the per-direction width
int run_hostlink_duplex_kernel(Rank& me, int my_rank, int host_rank, XferArgs& a, double t_call, mpx_timing* t) {
    return run_hostlink_call(me, my_rank, host_rank, a, a.nwg, kProtoHostDuplex, t_call, t,
                             [&] { return launch_hostlink_duplex(a, me.stream); });
}

// Start the armed call: one host store; the kernel has been waiting for it.
int start_armed(Rank& me, int my_rank, int peer_rank, int mode, int group, int iters, long long len,
                const mpx_xfer_opts* o, double t_call, mpx_timing* t) {
    KernelCall& kc = *me.armed;
    if (!armed_matches(kc, mode, group, peer_rank, iters, len, o))
        return fail(MPX_ERR_STATE, "rank %d is armed for another call (disarm it first)", my_rank);
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    kc.c.t0 = now_s();
    __atomic_store_n(&me.status->go, kc.a.go_token, __ATOMIC_RELEASE);
    const int st = complete_pair(me, kc, t_call, t);
    delete me.armed;
    me.armed = nullptr;
    return st;
}

// An armed call ends without a transfer: go = token | kGoCancel, wait for
// the kernel, and the call number it took back (the peer never saw it: the
// kernel exits before posting its receives).
int disarm(Rank& me) {
    if (!me.armed) return MPX_OK;
    KernelCall& kc = *me.armed;
    __atomic_store_n(&me.status->go, kc.a.go_token | kGoCancel, __ATOMIC_RELEASE);
    double t_done = 0;
    const int st = wait_kernel(me, kc.c.token, true, &t_done);
    give_back(me, kc.c, true);
    delete me.armed;
    me.armed = nullptr;
    return st;
}

}  // namespace mpx

extern "C" {

constexpr double kArmReadyWaitS = 5e-3;

int mpx_xfer_arm(mpx_ctx* ctx, int mode, int my_group, int my_rank, int peer_rank, int iters, void* tx, void* rx,
                 int buff_len, const mpx_xfer_opts* opts) {
    if (!ctx) return fail(MPX_ERR_INVALID, "NULL argument");
    TRY(check_call(ctx, mode, my_group, my_rank, peer_rank, iters, tx, rx, buff_len, opts));
    if (ctx->engine != MPX_ENGINE_KERNEL) return MPX_OK;   // nothing to launch ahead (include/mpx.h)
    Rank& me = ctx->r[my_rank];
    Rank& peer = ctx->r[peer_rank];
    if (me.armed) return fail(MPX_ERR_STATE, "rank %d is already armed (start or disarm it first)", my_rank);
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    KernelCall* kc = new KernelCall;
    int st = prepare_call(ctx, me, peer, my_rank, peer_rank, mode, my_group, iters, buff_len, opts, kc);
    if (st != MPX_OK) {
        delete kc;
        return st;
    }
    kc->c.armed = true;
    __atomic_store_n(&me.status->ready, 0ull, __ATOMIC_RELAXED);
    kc->a.go_token = kc->a.done_token;
    // the host's barrier sits between arm and start: bounded generously
    kc->a.go_timeout_ticks = std::max<u64>(kc->a.timeout_ticks, 60ull * 100000000ull);
    st = launch_call(me, kc->c, [&] { return launch_xfer(kc->a, kc->grid, me.stream); });
    if (st != MPX_OK) {
        // not launched: give the numbers back, and the inline call the
        // caller falls back to posts the one the peer waits for.  Launched
        // (a failure after the enqueue): the kernel waits for a go it will
        // never get — cancel it as disarm does, which also returns the call
        // number (the kernel exits before posting its receives)
        if (kc->c.launched) {
            me.armed = kc;
            (void)disarm(me);
        } else {
            give_back(me, kc->c);
            delete kc;
        }
        return st;
    }
    // Until the whole grid runs (Status.ready), a start would also wait for
    // the rest of the launch (the dispatch of every workgroup, ~5-10 us after
    // the launch call): wait for it here, ahead of the host's barrier.  The
    // wait is bounded (a grid that cannot all be resident yet, e.g. ranks
    // sharing a busy GPU, still starts correctly, only later).
    const double until = now_s() + kArmReadyWaitS;
    while (!(kc->c.resident = __atomic_load_n(&me.status->ready, __ATOMIC_ACQUIRE) == kc->a.go_token) && now_s() < until)
        cpu_relax();
    me.armed = kc;
    return MPX_OK;
}

int mpx_xfer_disarm(mpx_ctx* ctx, int my_rank) {
    if (!ctx) return fail(MPX_ERR_INVALID, "NULL argument");
    if (my_rank < 0 || my_rank >= ctx->nranks || !ctx->r[my_rank].local)
        return fail(MPX_ERR_STATE, "rank %d is not a local rank", my_rank);
    Rank& me = ctx->r[my_rank];
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    return disarm(me);
}

// ---------------------------------------------------------------------------
// fan exchange (include/mpx.h mpx_xfer_fan; k_xfer_fan, and k_xfer_fan_ll for
// MPX_FAN_LL)
// ---------------------------------------------------------------------------
namespace {
// MPX_FAN_WG: every link's width (read per call; every rank of a job inherits
// the same environment, so both sides of a link agree)
int fan_env_nwg() {
    const char* v = getenv("MPX_FAN_WG");
    return v ? atoi(v) : 0;
}

// The width of one fan link: the call's option, else MPX_FAN_WG, else the
// default rule; narrowed like a pair's (link_nwg).  0: invalid.
int fan_link_nwg(int nwg_opt, long long block_len, bool same_dev, int nranks) {
    return link_nwg(nwg_opt, fan_env_nwg(), fan_default_nwg(block_len, same_dev, nranks), block_len);
}

// The rank's fan table: device memory the kernel reads and folds its link
// results into, and its pinned host image (allocated on the first fan call;
// hipMalloc, unlike hipFree, does not wait for other ranks' kernels).
int ensure_fan_table(Rank& me) {
    if (me.fan_tab) return MPX_OK;
    void* h = nullptr;
    HIPCK(hipHostMalloc(&h, sizeof(FanTable), hipHostMallocDefault));
    void* d = nullptr;
    const hipError_t e = hipMalloc(&d, sizeof(FanTable));
    if (e != hipSuccess) {
        (void)hipHostFree(h);
        HIPCK(e);
    }
    me.fan_host = static_cast<FanTable*>(h);
    me.fan_tab = static_cast<FanTable*>(d);
    return MPX_OK;
}
}  // namespace

int mpx_fan_width(int nranks, int block_len, int same_device, int nwg) {
    if (nranks < 2 || nranks > MPX_MAX_RANKS || block_len < 0 || nwg < 0) return -1;
    const int w = fan_link_nwg(nwg, block_len, same_device != 0, nranks);
    return w > 0 ? w : -1;
}

namespace {
// what a sequenced fan call (mpx_xfer_fan_seq) adds to an ordinary one
struct FanSeq {
    u64 seed;                 // the job's seed: link k's pushes carry mpx_pattern_key(seed, me, peers[k], i)
    const uint64_t* expect;   // check mode: [npeers * iters], or null: computed here on the CPU
};

// One call path for mpx_xfer_fan (sq == null) and mpx_xfer_fan_seq: the same
// checks in the same order, table, lifecycle and results.  A sequenced call
// differs in the kernels' payload source (FanArgs.seq, seq_seed), in a
// per-payload expectation array for the verdict, and in never being traced.
int fan_call(mpx_ctx* ctx, int my_rank, int npeers, const int* peers, int iters, void* tx, void* rx, int block_len,
             size_t stride, const mpx_fan_opts* opts, mpx_timing* t, mpx_fan_link* links, const FanSeq* sq) {
    if (!ctx || !peers || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    memset(t, 0, sizeof *t);
    double t_call = now_s();
    // ---- argument checks: all before any GPU work ---------------------------
    if (my_rank < 0 || my_rank >= ctx->nranks) return fail(MPX_ERR_INVALID, "rank %d", my_rank);
    if (npeers < 1 || npeers > ctx->nranks - 1)
        return fail(MPX_ERR_INVALID, "npeers %d not in [1, %d]", npeers, ctx->nranks - 1);
    if (links) memset(links, 0, (size_t)npeers * sizeof *links);
    if (iters < 0 || block_len < 0) return fail(MPX_ERR_INVALID, "iters %d, block_len %d", iters, block_len);
    if ((long long)npeers * iters > 0x7fffffffll) return fail(MPX_ERR_INVALID, "npeers x iters %d x %d", npeers, iters);
    if (stride % 16 != 0 || stride < (size_t)block_len)
        return fail(MPX_ERR_INVALID, "stride %zu: a multiple of 16, at least block_len %d", stride, block_len);
    if (opts && (opts->flags & ~(MPX_XFER_STREAM | MPX_FAN_LL)))
        return fail(MPX_ERR_INVALID, "flags %#x: only MPX_XFER_STREAM or MPX_FAN_LL", opts->flags);
    const bool ll = opts && (opts->flags & MPX_FAN_LL);
    const bool check = opts && opts->check;
    if (check && !sq && !opts->expect_checksum) return fail(MPX_ERR_INVALID, "check mode needs expect_checksum[npeers]");
    bool seen[MPX_MAX_RANKS] = {};
    int top = my_rank;
    for (int k = 0; k < npeers; ++k) {
        const int p = peers[k];
        if (p < 0 || p >= ctx->nranks) return fail(MPX_ERR_INVALID, "peer rank %d", p);
        if (p == my_rank) return fail(MPX_ERR_INVALID, "rank %d lists itself as a peer", my_rank);
        if (seen[p]) return fail(MPX_ERR_INVALID, "peer rank %d listed twice", p);
        seen[p] = true;
        if (p > top) top = p;
    }
    if (ctx->engine != MPX_ENGINE_KERNEL)
        return fail(MPX_ERR_UNSUPPORTED, "%s: the kernel engine only", sq ? "mpx_xfer_fan_seq" : "mpx_xfer_fan");
    TRY(check_rank_state(ctx, my_rank, tx, rx, peers, npeers));
    Rank& me = ctx->r[my_rank];
    if (me.armed) return fail(MPX_ERR_STATE, "rank %d holds an armed call (start or disarm it first)", my_rank);
    if ((size_t)(top + 1) * stride > me.len)
        return fail(MPX_ERR_INVALID, "block %d at stride %zu lies past rank %d's attached length %zu", top, stride, my_rank,
                    me.len);
    // MPX_FAN_LL: a lock-step exchange of LL granules, one workgroup per link
    if (ll) {
        if (block_len > MPX_FAN_LL_MAX)
            return fail(MPX_ERR_INVALID, "MPX_FAN_LL: block_len %d above MPX_FAN_LL_MAX %d", block_len, MPX_FAN_LL_MAX);
        if (opts->flags & MPX_XFER_STREAM)
            return fail(MPX_ERR_INVALID, "MPX_FAN_LL with MPX_XFER_STREAM: an LL call has no bulk stores to stream");
        if (opts->nwg > 1) return fail(MPX_ERR_INVALID, "MPX_FAN_LL: nwg %d (an LL link is one workgroup wide)", opts->nwg);
    }
    int nwg[MPX_MAX_RANKS];
    for (int k = 0; k < npeers; ++k) {
        const Rank& peer = ctx->r[peers[k]];
        if ((size_t)(my_rank + 1) * stride > peer.len)
            return fail(MPX_ERR_INVALID, "block %d at stride %zu lies past rank %d's attached length %zu", my_rank, stride,
                        peers[k], peer.len);
        // (MPX_FAN_WG is not read for an LL call: its width is 1 by definition)
        nwg[k] = ll ? 1 : fan_link_nwg(opts ? opts->nwg : 0, block_len, same_device(me, peer), ctx->nranks);
        if (nwg[k] < 1) return fail(MPX_ERR_INVALID, "nwg > %d", kMaxPushWG);
    }
    std::vector<FanTable> image(1);
    FanTable& ht = image[0];
    memset(&ht, 0, sizeof ht);
    const int grid = fan_build_map(&ht, npeers, nwg, iters);
    if (grid < 0) {
        long long sum = 0;
        for (int k = 0; k < npeers; ++k) sum += nwg[k];
        return fail(MPX_ERR_INVALID, "rank %d: a fan grid of %lld workgroups exceeds %d (narrow the links: nwg, MPX_FAN_WG)",
                    my_rank, sum, kFanMaxGrid);
    }
    // a sequenced call's expectations the caller left to the library: on the
    // CPU (csrc/mpx_seq.h), before the timed part of the call
    std::vector<uint64_t> own;
    const uint64_t* want_each = nullptr;
    if (sq && check) {
        want_each = sq->expect;
        if (!want_each) {
            const u64 total = (u64)npeers * (u64)iters * (u64)block_len;
            if (total > MPX_SEQ_AUTO_MAX)
                return fail(MPX_ERR_INVALID,
                            "expect == NULL with %d x %d x %d B to generate on the CPU: above MPX_SEQ_AUTO_MAX (%llu)", npeers,
                            iters, block_len, (u64)MPX_SEQ_AUTO_MAX);
            own.resize((size_t)npeers * (size_t)iters);
            for (int k = 0; k < npeers; ++k) {
                const u64 base = seq::key_base(sq->seed, peers[k], my_rank);
                for (int i = 0; i < iters; ++i)
                    own[(size_t)k * iters + i] = seq::expect(seq::key_of(base, i), (size_t)block_len);
            }
            want_each = own.data();
            t_call = now_s();
        }
    }
    // ---- set-up ----------------------------------------------------------------
    DeviceGuard g(me.dev);
    HIPCK(g.err);
    TRY(ensure_fan_table(me));
    const size_t nsum = (size_t)npeers * (size_t)iters;
    if (check) TRY(ensure_csum(me, (int)nsum));
    const TestKnobs knobs = test_knobs();
    FanArgs a{};
    a.tx = me.tx;
    a.rx = me.rx;
    a.my_mb = me.mb;
    a.status = me.status;
    a.csum = me.csum;
    a.gbar = me.scratch;
    a.tab = me.fan_tab;
    a.timeout_ticks = timeout_ticks_ms(opts ? opts->timeout_ms : 0);
    a.len = block_len;
    a.iters = iters;
    a.nlinks = npeers;
    a.my_slot = my_rank;
    a.check = check ? 1 : 0;
    a.stream = (opts && (opts->flags & MPX_XFER_STREAM)) ? 1 : 0;
    a.nb_publish = nb_publish();
    a.skip_push = knobs.skip_push;
    a.seq = sq ? 1 : 0;
    a.seq_seed = sq ? sq->seed : 0;
    Call c;
    c.my_rank = my_rank;
    c.iters = iters;
    c.kernel = ll ? "LL fan kernel" : "fan kernel";
    c.fail_launch = knobs.fail_launch == my_rank;
    c.protocol = ll ? kProtoFanLL : kProtoFan;
    c.csum_words = check ? nsum : 0;
    c.table = &ht;
    // the call's numbers: the rank's token, and a call number on every link
    u64 call[MPX_MAX_RANKS];
    take_numbers(me, c, peers, npeers, knobs.no_posted, call);
    a.done_token = c.token;
    for (int k = 0; k < npeers; ++k) {
        const int p = peers[k];
        const Rank& peer = ctx->r[p];
        FanLink& l = ht.link[k];
        l.peer_rx = peer.rx + (size_t)my_rank * stride;
        l.peer_mb = peer.mb;
        l.tx_seq0 = me.tx_seq[p];
        l.rx_seq0 = me.rx_seq[p];
        l.call = call[k];
        l.off = (long long)((size_t)p * stride);
        l.peer = p;
        l.recv_done = ~0ull;
        l.t_end = 0;
        if (nwg[k] > c.nwg) c.nwg = nwg[k];   // reported: the widest link
    }
    // ---- the shared steps: launch, completion, check-mode verdict ---------------
    FanLLArgs la{};   // (MPX_FAN_LL: the grid is npeers, workgroup k is link k)
    if (ll) {
        la.f = a;
        if (knobs.lag_rank == my_rank && knobs.lag_us > 0) {
            la.lag_link = knobs.lag_wg < 0 ? knobs.lag_wg + npeers : knobs.lag_wg;
            la.lag_ticks = (u64)knobs.lag_us * 100ull;   // s_memrealtime: 100 MHz
        }
        // the link recorder (mpx_fan_lat_enable): launch_fan_ll then picks the traced kernels
        // (a sequenced call runs untraced whatever the recorder's state, and leaves its contents)
        la.lat = me.fan_lat.on && !sq ? me.fan_lat.base : nullptr;
        la.lat_stride = me.fan_lat.stride();
    }
    const int lst = launch_call(me, c, [&] { return ll ? launch_fan_ll(la, me.stream) : launch_fan(a, grid, me.stream); });
    if (lst != MPX_OK) {
        give_back(me, c);
        return lst;
    }
    t->bytes = 2ull * (uint64_t)block_len * (uint64_t)iters * (uint64_t)npeers;
    Fin fin{};
    TRY(complete_call(me, c, peers, npeers, t_call, t, &fin, [&](unsigned iteration) {
        if (ll)
            return fail(MPX_ERR_TIMEOUT,
                        "rank %d: a device wait of the lock-step LL fan exchange timed out at iteration %u (%d B with %d peers; "
                        "both ends of a link must set MPX_FAN_LL alike)",
                        my_rank, iteration, block_len, npeers);
        return fail(MPX_ERR_TIMEOUT, "rank %d: a device wait of the fan exchange timed out at iteration %u (%d B to %d peers)",
                    my_rank, iteration, block_len, npeers);
    }));
    // the link results ride on the verdict's synchronise of the rank's stream
    HIPCK(hipMemcpyAsync(me.fan_host->link, me.fan_tab->link, (size_t)npeers * sizeof(FanLink), hipMemcpyDeviceToHost,
                         me.stream));
    int bad[MPX_MAX_RANKS] = {};
    u64 digest[MPX_MAX_RANKS] = {};
    const int verdict = check_verdict(me, my_rank, check ? npeers : 0, iters, (u64)block_len,
                                      check && !sq ? opts->expect_checksum : nullptr, t, bad, digest, want_each);
    if (verdict != MPX_OK && verdict != MPX_ERR_CHECK) return verdict;
    for (int k = 0; links && k < npeers; ++k) {
        const FanLink& l = me.fan_host->link[k];
        links[k].peer = peers[k];
        links[k].nwg = nwg[k];
        links[k].recv_done = l.recv_done == ~0ull ? 0 : l.recv_done;
        links[k].recv_digest = digest[k];
        links[k].check_failures = bad[k];
        links[k].device_s = (fin.t_entry && l.t_end >= fin.t_entry) ? (double)(l.t_end - fin.t_entry) * 1e-8 : 0;
    }
    return verdict;
}
}  // namespace

int mpx_xfer_fan(mpx_ctx* ctx, int my_rank, int npeers, const int* peers, int iters, void* tx, void* rx,
                 int block_len, size_t stride, const mpx_fan_opts* opts, mpx_timing* t, mpx_fan_link* links) {
    return fan_call(ctx, my_rank, npeers, peers, iters, tx, rx, block_len, stride, opts, t, links, nullptr);
}

// sequenced fan payloads (include/mpx_fan_seq.h; k_xfer_fan's and k_xfer_fan_ll's GEN instantiations)
int mpx_xfer_fan_seq(mpx_ctx* ctx, int my_rank, int npeers, const int* peers, int iters, void* tx, void* rx,
                     int block_len, size_t stride, const mpx_fan_seq_opts* opts, mpx_timing* t, mpx_fan_link* links) {
    if (!ctx || !peers || !opts || !t) return fail(MPX_ERR_INVALID, "NULL argument");
    mpx_fan_opts o{};
    o.check = opts->check ? 1 : 0;
    o.flags = opts->flags;   // (fan_call refuses any bit other than MPX_XFER_STREAM / MPX_FAN_LL)
    o.timeout_ms = opts->timeout_ms;
    o.nwg = opts->nwg;
    const FanSeq sq{opts->seed, opts->expect};
    return fan_call(ctx, my_rank, npeers, peers, iters, tx, rx, block_len, stride, &o, t, links, &sq);
}

}  // extern "C"
