// stream_loop_check — the stream engines' one loop (mpx_stream_loop.h) run on
// the CPU with a recording operations object: a stand-alone program (plain
// g++, or tools/asan_fan.sh's sanitizer build; no GPU, no libmpx; run once by
// tests/test_tools.py).  The recorder has four personalities, one per
// operations object of mpx_engine_stream.hip, that differ only in what a hook
// expands to; each primitive it "enqueues" is appended as (op, n, i, publish,
// lost) and counted as the engine counts mpx_timing.launches.  Checked, the
// first mismatch prints and exits 1:
//   * exact sequences: 3 modes x 2 sides at iters = 2 against lists written
//     out below from the four ladders the loop replaced (SdmaOps::step,
//     pull_step, nb_checked and run_rccl of the commit before it);
//   * the non-blocking window's arithmetic at iters 1 .. 600;
//   * the publish schedule at nb_publish 1, 16, 256;
//   * that a captured chunk plus the rest equals the loop run in one piece.
// `stream_loop_check counts` prints what the pytest side compares with
// tests/stream_launches.py and tests/golden/ref_runs.json.
#include "mpx_stream_loop.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace mpx;

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

enum Kind { PUSH, PULL, NBCHECK, RCCL };
static const char* const kKindName[] = {"push", "pull", "nbcheck", "rccl"};

// one primitive: i is the iteration (copy, check, RCCL calls), the push number
// relative to the call's base (flag / ready / credit stores and waits), or the
// first receive (account, with its count)
struct Rec {
    const char* op;
    long long n;
    int i;
    bool publish, lost;
    int count;
};

struct Recorder {
    explicit Recorder(Kind k) : kind(k) {}
    Kind kind;
    int iters = 0, slots = kNbWindow;        // NBCHECK's
    std::vector<Rec> t;
    std::vector<std::pair<int, int>> flushes;   // (i, inflight) of every nb_flush
    int launches = 0;
    bool pub = true, lst = false;             // of the hook being expanded

    void prim(const char* op, long long n, int i, bool counted = true, int count = 0) {
        t.push_back({op, n, i, pub, lst, count});
        if (counted) ++launches;
    }
    void copy(long long n, int i) {
        if (n > 0 && !lst) prim("copy", n, i);   // a skipped or zero-byte copy is not enqueued
    }
    void hook(bool publish, bool lost) { pub = publish, lst = lost; }

    int send(long long n, int i, bool publish, bool lost, bool ack) {
        hook(publish, lost);
        if (kind == RCCL) {
            prim("rsend", n, i);
        } else if (kind == PULL && !ack) {
            prim("ready", 0, i + 1);
        } else {
            if (kind == PULL) lst = false;       // the pushed ack of a pulled call is never lost
            copy(n, i);
            if (publish) prim("flag", 0, i + 1);
        }
        return MPX_OK;
    }
    int recv(long long n, int i, bool publish, bool lost, bool ack) {
        hook(publish, lost);
        if (kind == RCCL) {
            prim("rrecv", n, i);
        } else if (kind == PULL && !ack) {
            prim("wready", 0, i + 1);
            copy(n, i);
            if (publish) prim("credit", 0, i + 1);
        } else {
            prim("wflag", 0, i + 1);
        }
        return MPX_OK;
    }
    int nb_post(long long n, int i, bool publish, bool lost) {
        hook(publish, lost);
        if (kind == RCCL) {
            prim("group", n, i);
        } else if (kind == PULL) {
            send(n, i, true, false, false);
            recv(n, i, publish, lost, false);
        } else if (kind == NBCHECK) {
            if (i >= slots) prim("wcredit", 0, i - slots + 1);
            copy(n, i);
            prim("flag", 0, i + 1);
            prim("wflag", 0, i + 1);
        } else {
            send(n, i, publish, lost, false);
        }
        return MPX_OK;
    }
    int nb_flush(int i, int inflight) {
        hook(true, false);
        flushes.push_back({i, inflight});
        if (kind == PUSH) prim("wflag", 0, i);
        if (kind == PULL) prim("wcredit", 0, i);
        return MPX_OK;
    }
    int check(long long n, int i, int) {
        hook(true, false);
        if (n > 0) prim("check", n, i, false);
        if (kind == NBCHECK) prim("credit", 0, i + 1);
        return MPX_OK;
    }
    int account(int j0, int count, long long n) {
        hook(true, false);
        prim("account", n, j0, false, count);
        return MPX_OK;
    }
    int drain(const StreamCall& c, int inflight) {
        hook(true, false);
        if (kind == PUSH && c.mode == MPX_MODE_NONBLOCKING && inflight > 0) prim("wflag", 0, c.iters);
        if (kind == PULL && (c.mode != MPX_MODE_UNIDIR || c.group == 1)) prim("wcredit", 0, c.iters);
        return MPX_OK;
    }
};

static std::string text(const std::vector<Rec>& t, bool drop_checks = false) {
    std::string s;
    for (const Rec& r : t) {
        const bool is_check = !strcmp(r.op, "check") || !strcmp(r.op, "account");
        if (drop_checks && is_check) continue;
        const bool sized = is_check || !strcmp(r.op, "copy") || !strcmp(r.op, "rsend") || !strcmp(r.op, "rrecv") ||
                           !strcmp(r.op, "group");
        char b[96];
        if (!strcmp(r.op, "account")) snprintf(b, sizeof b, "account:%lld:%d+%d", r.n, r.i, r.count);
        else if (sized) snprintf(b, sizeof b, "%s:%lld:%d", r.op, r.n, r.i);
        else snprintf(b, sizeof b, "%s:%d", r.op, r.i);
        if (!s.empty()) s += ' ';
        s += b;
        if (r.lost) s += "(lost)";
    }
    return s;
}

// the loop and its tail over [i0, iters) of one call
static Recorder run(Kind kind, int mode, int group, long long len, int iters, bool check, int nbp = 16, int skip = 0,
                    int i0 = 0, int inflight0 = 0) {
    Recorder r(kind);
    r.iters = iters;
    const StreamCall c{mode, group, len, iters, check, nbp, skip};
    int inflight = inflight0;
    if (stream_loop(r, c, i0, iters, &inflight) != MPX_OK || stream_tail(r, c, inflight) != MPX_OK) r.launches = -1;
    return r;
}

// ---- exact sequences --------------------------------------------------------
// B = 5 bytes, 2 iterations, check mode; copy:n:i check:n:i account:n:first+count
// rsend/rrecv/group:n:i; flag, ready, credit (stores) and wflag, wready, wcredit
// (waits) carry the push number relative to the call's base.  With check off
// the list is the same without its check and account entries (`if (check)` in
// every ladder).  The non-blocking loop is the same on both sides.
struct Want {
    Kind kind;
    int mode, group;
    bool check;
    const char* ops;
};
static const Want kWant[] = {
    // SdmaOps::step
    {PUSH, MPX_MODE_PINGPONG, 1, true,
     "copy:5:0 flag:1 wflag:1 check:5:0 copy:5:1 flag:2 wflag:2 check:5:1 account:5:0+2"},
    {PUSH, MPX_MODE_PINGPONG, 0, true,
     "wflag:1 check:5:0 copy:5:0 flag:1 wflag:2 check:5:1 copy:5:1 flag:2 account:5:0+2"},
    {PUSH, MPX_MODE_UNIDIR, 1, true,
     "copy:5:0 flag:1 wflag:1 check:1:0 copy:5:1 flag:2 wflag:2 check:1:1 account:1:0+2"},
    {PUSH, MPX_MODE_UNIDIR, 0, true,
     "wflag:1 check:5:0 copy:1:0 flag:1 wflag:2 check:5:1 copy:1:1 flag:2 account:5:0+2"},
    // push 1 is not published (schedule: every 16th, slot 254, the last); run_sdma's final wait
    {PUSH, MPX_MODE_NONBLOCKING, 1, false, "copy:5:0 copy:5:1 flag:2 wflag:2"},
    // SdmaOps::pull_step, and run_sdma's wait_pulled before the blocking loops' account, after the window's
    {PULL, MPX_MODE_PINGPONG, 1, true,
     "ready:1 wready:1 copy:5:0 credit:1 check:5:0 ready:2 wready:2 copy:5:1 credit:2 check:5:1 wcredit:2 "
     "account:5:0+2"},
    {PULL, MPX_MODE_PINGPONG, 0, true,
     "wready:1 copy:5:0 credit:1 check:5:0 ready:1 wready:2 copy:5:1 credit:2 check:5:1 ready:2 wcredit:2 "
     "account:5:0+2"},
    {PULL, MPX_MODE_UNIDIR, 1, true, "ready:1 wflag:1 check:1:0 ready:2 wflag:2 check:1:1 wcredit:2 account:1:0+2"},
    {PULL, MPX_MODE_UNIDIR, 0, true,
     "wready:1 copy:5:0 credit:1 check:5:0 copy:1:0 flag:1 wready:2 copy:5:1 credit:2 check:5:1 copy:1:1 flag:2 "
     "account:5:0+2"},
    {PULL, MPX_MODE_NONBLOCKING, 1, true,
     "ready:1 wready:1 copy:5:0 check:5:0 ready:2 wready:2 copy:5:1 credit:2 check:5:1 account:5:0+2 wcredit:2"},
    // SdmaOps::nb_checked (check mode only)
    {NBCHECK, MPX_MODE_NONBLOCKING, 1, true,
     "copy:5:0 flag:1 wflag:1 check:5:0 credit:1 copy:5:1 flag:2 wflag:2 check:5:1 credit:2 account:5:0+2"},
    // run_rccl
    {RCCL, MPX_MODE_PINGPONG, 1, true,
     "rsend:5:0 rrecv:5:0 check:5:0 rsend:5:1 rrecv:5:1 check:5:1 account:5:0+2"},
    {RCCL, MPX_MODE_PINGPONG, 0, true,
     "rrecv:5:0 check:5:0 rsend:5:0 rrecv:5:1 check:5:1 rsend:5:1 account:5:0+2"},
    {RCCL, MPX_MODE_UNIDIR, 1, true, "rsend:5:0 rrecv:1:0 check:1:0 rsend:5:1 rrecv:1:1 check:1:1 account:1:0+2"},
    {RCCL, MPX_MODE_UNIDIR, 0, true, "rrecv:5:0 check:5:0 rsend:1:0 rrecv:5:1 check:5:1 rsend:1:1 account:5:0+2"},
    {RCCL, MPX_MODE_NONBLOCKING, 1, true, "group:5:0 check:5:0 group:5:1 check:5:1 account:5:0+2"},
};

static int same(const std::string& got, const std::string& want, const Want& w, int group, bool check) {
    if (got == want) return 0;
    fprintf(stderr, "%s mode %d group %d check %d:\n  got  %s\n  want %s\n", kKindName[w.kind], w.mode, group, check,
            got.c_str(), want.c_str());
    return 1;
}

static int check_sequences() {
    for (const Want& w : kWant) {
        const bool nb = w.mode == MPX_MODE_NONBLOCKING;
        for (int group = nb ? 0 : w.group; group <= (nb ? 1 : w.group); ++group) {
            const Recorder on = run(w.kind, w.mode, group, 5, 2, w.check);
            if (same(text(on.t), w.ops, w, group, w.check)) return 1;
            if (!w.check || w.kind == NBCHECK) continue;
            const Recorder off = run(w.kind, w.mode, group, 5, 2, false);
            if (same(text(off.t), text(on.t, true), w, group, false)) return 1;
        }
    }
    // the lost payload (skip_push = 1): the side that copies skips its copy and
    // still signals; RCCL's send carries rx; the pushed ack of a pulled call is sent
    REQUIRE(text(run(PUSH, MPX_MODE_PINGPONG, 1, 5, 1, false, 16, 1).t) == "flag:1(lost) wflag:1(lost)");
    REQUIRE(text(run(PUSH, MPX_MODE_UNIDIR, 0, 5, 1, false, 16, 1).t) == "wflag:1(lost) flag:1(lost)");
    REQUIRE(text(run(PULL, MPX_MODE_PINGPONG, 1, 5, 1, false, 16, 1).t) ==
            "ready:1(lost) wready:1(lost) credit:1(lost) wcredit:1");
    REQUIRE(text(run(PULL, MPX_MODE_UNIDIR, 0, 5, 1, false, 16, 1).t) ==
            "wready:1(lost) credit:1(lost) copy:1:0 flag:1");
    REQUIRE(text(run(NBCHECK, MPX_MODE_NONBLOCKING, 1, 5, 1, true, 16, 1).t) ==
            "flag:1(lost) wflag:1(lost) check:5:0 credit:1 account:5:0+1");
    REQUIRE(text(run(RCCL, MPX_MODE_NONBLOCKING, 0, 5, 1, false, 16, 1).t) == "group:5:0(lost)");
    REQUIRE(text(run(RCCL, MPX_MODE_UNIDIR, 0, 5, 1, false, 16, 1).t) == "rrecv:5:0(lost) rsend:1:0(lost)");
    // no iteration: nothing at all
    for (Kind k : {PUSH, PULL, NBCHECK, RCCL})
        for (int mode = MPX_MODE_PINGPONG; mode <= MPX_MODE_UNIDIR; ++mode) REQUIRE(run(k, mode, 1, 5, 0, true).t.empty());
    return 0;
}

// ---- the window -------------------------------------------------------------
static const int kWindowIters[] = {1, 254, 255, 256, 257, 512, 600};

// receives the accounting of a checked non-blocking call counts, or -1
static long long accounted(const Recorder& r, int iters) {
    std::vector<char> seen((size_t)iters, 0);
    long long sum = 0;
    for (const Rec& a : r.t) {
        if (strcmp(a.op, "account")) continue;
        if (a.i < 0 || a.count <= 0 || a.i + a.count > iters) return -1;
        for (int j = a.i; j < a.i + a.count; ++j) {
            if (seen[(size_t)j]) return -1;                                        // ranges are disjoint
            if (j % kNbWindow == kNbWindow - 1 && j < iters / kNbWindow * kNbWindow) return -1;   // never a full window's slot 255
            seen[(size_t)j] = 1;
        }
        sum += a.count;
    }
    return sum;
}

static int check_window() {
    for (Kind k : {PUSH, PULL, NBCHECK, RCCL})
        for (int iters : kWindowIters)
            for (int check = 0; check <= 1; ++check) {
                if ((k == PUSH && check) || (k == NBCHECK && !check)) continue;   // never run so
                const Recorder r = run(k, MPX_MODE_NONBLOCKING, 1, 64, iters, check != 0);
                // a flush exactly at every i = 255 (mod 256), of 255 requests
                REQUIRE((int)r.flushes.size() == iters / kNbWindow);
                for (size_t f = 0; f < r.flushes.size(); ++f)
                    REQUIRE(r.flushes[f].first == (int)f * kNbWindow + kNbWindow - 1 && r.flushes[f].second == kNbWindow - 1);
                REQUIRE(accounted(r, iters) == (check ? iters - iters / kNbWindow : 0));
            }
    return 0;
}

// ---- the publish schedule ---------------------------------------------------
static int check_publish() {
    for (int nbp : {1, 16, 256})
        for (int iters : kWindowIters) {
            const Recorder r = run(PUSH, MPX_MODE_NONBLOCKING, 0, 64, iters, false, nbp);
            int copies = 0;
            for (const Rec& c : r.t) {
                if (strcmp(c.op, "copy")) continue;
                const int i = c.i;
                const bool want = (i + 1) % nbp == 0 || i % 256 == 254 || i == iters - 1;   // restated
                REQUIRE(c.publish == want && want == nb_publishes(i, iters, nbp));
                ++copies;
            }
            REQUIRE(copies == iters);
            // the blocking modes publish every send
            for (int mode : {MPX_MODE_PINGPONG, MPX_MODE_UNIDIR})
                for (const Rec& c : run(PUSH, mode, 1, 64, iters, false, nbp).t) REQUIRE(c.publish);
        }
    return 0;
}

// ---- graph capture ----------------------------------------------------------
// What run_sdma does with graphs: a chunk captured as the range [0, count) of
// a call of `count` iterations (its push numbers relative to the device's
// sequence base, which the chunk advances by count), then the rest [count,
// iters) of the call enqueued plainly.  That equals the call enqueued in one
// piece — except that the chunk's last push, count - 1, is always published.
static int check_capture() {
    for (Kind k : {PUSH, PULL})
        for (int mode = MPX_MODE_PINGPONG; mode <= MPX_MODE_UNIDIR; ++mode)
            for (int group = 0; group <= 1; ++group)
                for (int count : {16, 100, 256})
                    for (int iters : {256, 257, 300, 600}) {
                        if (count > iters) continue;
                        Recorder chunk(k);
                        const StreamCall cc{mode, group, 64, count, false, 16, 0};
                        int inflight = 0;
                        REQUIRE(stream_loop(chunk, cc, 0, count, &inflight) == MPX_OK);
                        REQUIRE(inflight == (mode == MPX_MODE_NONBLOCKING ? count % kNbWindow : 0));
                        const Recorder rest = run(k, mode, group, 64, iters, false, 16, 0, count, inflight);
                        std::vector<Rec> two = chunk.t;
                        two.insert(two.end(), rest.t.begin(), rest.t.end());
                        const Recorder one = run(k, mode, group, 64, iters, false);
                        // the exception: push count - 1's flag (pull: credit) store, where the one piece has none
                        std::vector<Rec> want;
                        for (const Rec& r : two) {
                            const bool store = !strcmp(r.op, "flag") || !strcmp(r.op, "credit");
                            const bool extra = mode == MPX_MODE_NONBLOCKING && store && r.i == count &&
                                               !nb_publishes(count - 1, iters, 16);
                            if (!extra) want.push_back(r);
                        }
                        REQUIRE(text(want) == text(one.t));
                        const bool differs = mode == MPX_MODE_NONBLOCKING && !nb_publishes(count - 1, iters, 16);
                        REQUIRE((int)two.size() == (int)one.t.size() + (differs ? 1 : 0));
                        REQUIRE(chunk.launches + rest.launches == one.launches + (differs ? 1 : 0));
                    }
    return 0;
}

// ---- what tests/test_tools.py reads -------------------------------------------
// launches <pull> <mode> <group> <n> <iters> <check> <i0> <count>: what the
// SDMA engine's loop and tail enqueue after graph replays covering [0, i0);
// accounted <kind> <iters> <receives>: a checked non-blocking call's accounting
static int print_counts() {
    const int sizes[] = {0, 1, 4097};
    const int shapes[][2] = {{1, 0}, {3, 0}, {15, 0}, {255, 1}, {256, 1}, {257, 1}, {600, 0}};
    for (int pull = 0; pull <= 1; ++pull)
        for (int mode = MPX_MODE_PINGPONG; mode <= MPX_MODE_UNIDIR; ++mode)
            for (int group = 0; group <= 1; ++group)
                for (int n : sizes)
                    for (const auto& s : shapes) {
                        const int iters = s[0];
                        const bool check = s[1] != 0;
                        // run_sdma's split: 256-iteration chunks and a remainder of >= 16, unchecked calls only
                        int i0 = 0;
                        if (!check && iters >= 16) i0 = iters - (iters % 256 >= 16 ? 0 : iters % 256);
                        const Kind k = pull ? PULL : (check && mode == MPX_MODE_NONBLOCKING) ? NBCHECK : PUSH;
                        const Recorder r = run(k, mode, group, n, iters, check, 16, 0, i0, i0 % kNbWindow);
                        REQUIRE(r.launches >= 0);
                        printf("launches %d %d %d %d %d %d %d %d\n", pull, mode, group, n, iters, (int)check, i0, r.launches);
                    }
    for (Kind k : {PULL, NBCHECK, RCCL})
        for (int iters : kWindowIters)
            printf("accounted %s %d %lld\n", kKindName[k], iters,
                   accounted(run(k, MPX_MODE_NONBLOCKING, 0, 64, iters, true), iters));
    return 0;
}

int main(int argc, char** argv) {
    if (check_sequences() || check_window() || check_publish() || check_capture()) return 1;
    if (argc > 1 && !strcmp(argv[1], "counts")) return print_counts();
    puts("stream_loop_check: ok");
    return 0;
}
