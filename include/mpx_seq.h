/* mpx_seq.h - sequenced payloads: the pair loops with a payload of its own in
   every iteration.  Part of the C-ABI of include/mpx.h, which includes this
   file inside its extern "C" block: include "mpx.h", not this file. */
#ifndef MPX_SEQ_H
#define MPX_SEQ_H
#ifndef MPX_H
#error "include mpx.h: it includes mpx_seq.h where the types it needs are declared"
#endif

/* ---- sequenced payloads ------------------------------------------------------ */
/* mpx_xfer_ex re-sends the same tx in every iteration, as the reference does
   (mpi_perf.c:72,80,136), so a payload that arrives one iteration early or
   late, twice, or from a stale copy leaves the bytes it would have left
   anyway.  mpx_xfer_seq runs the same three loops with the payload
       P(seed, s, d, i, n) = the first n bytes mpx_fill(MPX_FILL_SPLITMIX,
                             mpx_pattern_key(seed, s, d, i)) writes
   as the message rank s sends to rank d in iteration i: n = buff_len, or 1 for
   the unidir ack (byte 0 of the acking rank's pattern of that iteration).  The
   pushing kernel generates the bytes in registers; tx is neither read nor
   written.  After any completed call, checked or not, rx[0 : recv_len) holds
   P(seed, peer, me, iters - 1, recv_len).
     Everything else is mpx_xfer_ex's on the kernel engine: modes, groups,
   argument checks, the LL / bulk choice, widths (nwg, MPX_PUSH_WG), the
   receive-posted handshake, the non-blocking window (recv_done counts the
   receives the reference completes: every i with i % 256 != 255), the check
   ring and its credits, mpx_timing (protocol 0 or 1, launches = 1),
   mpx_last_phases and the link counters.  So sequenced and ordinary calls may
   alternate on one link, and the two sides of a call need not agree: if only
   one side calls mpx_xfer_seq both calls complete, and the sequenced side
   receives the peer's tx bytes - which an unchecked call cannot notice.
     Check mode (check = 1): every received payload is checksummed and all
   but the last poisoned, as mpx_xfer_ex does; payload i is compared with
   expect[i], so check_iters = iters and check_failures counts the iterations
   that differ.  recv_digest is the sum of the finished checksums of the
   receives recv_done counts.  expect == NULL: the library computes the
   expectations on the CPU before the timed part of the call; refused when
   iters * recv_len exceeds MPX_SEQ_AUTO_MAX.
     Statuses, all decided before any GPU work:
       MPX_ERR_UNSUPPORTED  an SDMA or RCCL context; MPX_XFER_PULL=1 in the
                            environment (a pulled payload would have to be
                            written into tx first)
       MPX_ERR_INVALID      NULL ctx / opts / t; any flags bit other than
                            MPX_XFER_STREAM (no tx is read, so MPX_XFER_NOSTAGE
                            means nothing); whatever mpx_xfer_ex refuses
       MPX_ERR_STATE        a rank that holds an armed call (a sequenced call
                            cannot be armed), that timed out before, or that is
                            not attached here (a host endpoint included)
     Afterwards: MPX_ERR_TIMEOUT, MPX_ERR_CHECK.
     Sequenced calls are never traced by the latency recorder (mpx_lat_*),
   like non-blocking calls; peer_rank == my_rank is allowed for
   MPX_MODE_NONBLOCKING.  The ABI version is unchanged: callers detect the
   feature by symbol. */
#define MPX_SEQ_AUTO_MAX (1ull << 28)   /* bytes the library will generate on the CPU for expect == NULL */
typedef struct mpx_seq_opts {
    uint64_t seed;            /* both sides of a link pass the same seed            */
    int32_t  check;           /* 1: checksum + poison every received payload        */
    int32_t  flags;           /* 0 or MPX_XFER_STREAM                               */
    uint32_t timeout_ms;      /* as mpx_xfer_opts                                   */
    int32_t  nwg;             /* as mpx_xfer_opts                                   */
    const uint64_t *expect;   /* check = 1: [iters] checksums of the payloads this
                                 side receives, expect[i] = mpx_checksum value of
                                 P(seed, peer, me, i, recv_len); NULL: the library
                                 computes them on the CPU before the launch         */
} mpx_seq_opts;
int mpx_xfer_seq(mpx_ctx *ctx, int mode, int my_group, int my_rank, int peer_rank, int iters,
                 void *tx, void *rx, int buff_len, const mpx_seq_opts *opts, mpx_timing *t);
/* pure host, no ctx, no GPU: the checksum of P(seed, src, dst, iter, n).
   MPX_ERR_INVALID for a NULL out, a rank outside [0, MPX_MAX_RANKS) or a
   negative iter */
int mpx_seq_expect(uint64_t seed, int src, int dst, int iter, size_t n, uint64_t *out);

#endif /* MPX_SEQ_H */
