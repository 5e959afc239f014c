// mpx_stream_loop.h — the reference's transfer loop (mpi_perf.c:66-145: three
// modes x two sides, the 256-request window, Waitall(255) over slots 0..254,
// the final Waitall(inflight)), written once for the stream engines.  What an
// iteration enqueues is the engine's: the loop calls an operations object
//   send(n, i, publish, lost, ack)   the payload or ack send of iteration i
//   recv(n, i, publish, lost, ack)   the blocking receive of iteration i
//   nb_post(n, i, publish, lost)     Isend + Irecv of one non-blocking iteration
//   nb_flush(i, inflight)            Waitall(255) before iteration i + 1: pushes 0..i-1
//   check(n, i, iters)               checksum + poison the payload received in iteration i
//   account(j0, count, n)            the device counts receives [j0, j0 + count) of n bytes
//   drain(call, inflight)            what the engine itself still waits for at the call's end
// publish: the push is made visible to the peer (non-blocking schedule below;
// always in the blocking modes); lost: the test knob's payload that is not
// moved; ack: unidir's 1-byte reply.  No HIP call here: tools/stream_loop_check.cpp
// runs the loop on the CPU with a recording operations object.
#pragma once

#include "mpx_internal.h"

namespace mpx {

struct StreamCall {
    int mode, group;
    long long len;
    int iters;        // the call's iterations (graph capture: the chunk's)
    bool check;
    int nb_publish;   // nb_publish() of the runtime
    int skip;         // test knob: 1 + the iteration whose payload is lost; 0 = off
};

// non-blocking publish schedule shared by the kernel and SDMA engines: every
// `every` pushes, at window slot 254 (the last receive a Waitall(255) waits
// for, so no flush waits for the slot-255 push the reference leaves pending)
// and at the last push
inline bool nb_publishes(int i, int iters, int every) {
    return (i + 1) % every == 0 || i % kNbWindow == kNbWindow - 2 || i + 1 == iters;
}

// the side that receives unidir's acks: they are always 1 byte (mpi_perf.c:137,142)
inline bool ack_side(const StreamCall& c) { return c.mode == MPX_MODE_UNIDIR && c.group == 1; }

// Enqueues iterations [i0, i1) of the call (mpi_perf.c:70-82, 95-124,
// 132-144); *inflight is the non-blocking window's fill.  Check mode
// checksums + poisons each received payload where the reference's Recv
// returns (mpi_perf.c:75, 79, 137, 141): before group 0's reply / ack (:80, :142).
template <class Ops>
int stream_loop(Ops& op, const StreamCall& c, int i0, int i1, int* inflight) {
    const bool uni = c.mode == MPX_MODE_UNIDIR;
    const long long reply = uni ? 1 : c.len;   // Send(tx, 1): always one byte
    for (int i = i0; i < i1; ++i) {
        const bool lost = c.skip == i + 1;
        if (c.mode == MPX_MODE_NONBLOCKING) {
            TRY(op.nb_post(c.len, i, nb_publishes(i, c.iters, c.nb_publish), lost));
            if (c.check) TRY(op.check(c.len, i, c.iters));
            if (*inflight == kNbWindow - 1) {
                // Waitall(255): iterations i-255 .. i-1, not slot 255's receive
                TRY(op.nb_flush(i, *inflight));
                if (c.check) TRY(op.account(i - *inflight, *inflight, c.len));
                *inflight = 0;
            } else {
                ++*inflight;
            }
        } else if (c.group == 1) {
            TRY(op.send(c.len, i, true, lost, false));
            TRY(op.recv(reply, i, true, lost, uni));
            if (c.check) TRY(op.check(reply, i, c.iters));
        } else {
            TRY(op.recv(c.len, i, true, lost, false));
            if (c.check) TRY(op.check(c.len, i, c.iters));
            TRY(op.send(reply, i, true, lost, uni));
        }
    }
    return MPX_OK;
}

// The call's end, after its last iteration: the receives of the final
// Waitall(inflight) counted (mpi_perf.c:122-123), the engine's own last wait,
// and — every receive of ping-pong / unidir is complete then — those counted
// and their checksums digested.
template <class Ops>
int stream_tail(Ops& op, const StreamCall& c, int inflight) {
    if (c.iters <= 0) return MPX_OK;
    const bool nb = c.mode == MPX_MODE_NONBLOCKING;
    if (nb && c.check && inflight > 0) TRY(op.account(c.iters - inflight, inflight, c.len));
    TRY(op.drain(c, inflight));
    if (!nb && c.check) TRY(op.account(0, c.iters, ack_side(c) ? 1 : c.len));
    return MPX_OK;
}

}  // namespace mpx
