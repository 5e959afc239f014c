/* mpx_fan_seq.h - sequenced fan payloads: the fan exchange with a payload of
   its own per (sender, receiver, iteration).  Part of the C-ABI of
   include/mpx.h, which includes this file inside its extern "C" block:
   include "mpx.h", not this file. */
#ifndef MPX_FAN_SEQ_H
#define MPX_FAN_SEQ_H
#ifndef MPX_H
#error "include mpx.h: it includes mpx_fan_seq.h where the types it needs are declared"
#endif

/* ---- sequenced fan payloads --------------------------------------------------- */
/* mpx_xfer_fan pushes the same tx blocks in every iteration, so a block that
   arrives one iteration early or late, twice, from the other half of an LL row
   or from a stale copy leaves the bytes it would have left anyway.
   mpx_xfer_fan_seq runs the same exchange, bulk or MPX_FAN_LL, with mpx_seq.h's
   payload and no new arithmetic:
       in iteration i rank s pushes P(seed, s, d, i, block_len) into
       rx_d[s * stride : + block_len)
   for every peer d; word indices count from the block's start.  The pushing
   kernel generates the bytes in registers.
     Buffers: tx is neither read nor written.  No other byte of rx is written:
   the gaps, the rank's own block and the blocks of ranks outside the peer set
   all stay.  After a completed call, checked or not, rx block p holds
   P(seed, p, me, iters - 1, block_len) for every peer p.
     Everything else is mpx_xfer_fan's.  On the caller's side: peer sets,
   layout, argument checks and their order, widths (nwg, MPX_FAN_WG,
   mpx_fan_width).  In the protocol: the receive-posted word, the publish
   schedule, credits in check mode, MPX_FAN_LL's halves and its 4096-byte limit.
   In the results: mpx_timing (protocol 9 or 10, launches = 1), mpx_fan_link,
   the link counters.  So sequenced and ordinary fan calls, and pair calls of
   either kind, may alternate on a link, and the two ends of a link need not
   agree: if only one end is sequenced both calls complete, and the sequenced
   end receives the peer's tx block - which an unchecked call cannot notice.
     Check mode (check = 1): every received block is checksummed and all but the
   last poisoned, as mpx_xfer_fan does; payload i of link k (peers[k], the
   caller's order) is compared with expect[k * iters + i].
   links[k].check_failures counts that link's differing iterations,
   t->check_failures is their sum, check_iters = npeers * iters, and the
   digests are the sums of the finished checksums, as for mpx_xfer_fan.
   expect == NULL: the library computes the expectations on the CPU before the
   timed part of the call; refused (MPX_ERR_INVALID, as mpx_xfer_seq's own
   limit) when npeers * iters * block_len exceeds MPX_SEQ_AUTO_MAX.
     Statuses, all decided before any GPU work:
       MPX_ERR_INVALID      NULL ctx / peers / opts / t; any flags bit other
                            than MPX_XFER_STREAM / MPX_FAN_LL; the expect ==
                            NULL limit; whatever mpx_xfer_fan refuses
       MPX_ERR_UNSUPPORTED  a context of another engine than the kernel engine
       MPX_ERR_STATE        as mpx_xfer_fan
     Afterwards: MPX_ERR_TIMEOUT, MPX_ERR_CHECK.
     Recorder: a sequenced MPX_FAN_LL call on a rank whose link recorder
   (mpx_fan_lat_*) is enabled runs untraced and leaves the recorder's contents
   as they were; sequenced pair calls treat mpx_lat_* the same way.  The ABI
   version is unchanged: callers detect the feature by symbol. */
typedef struct mpx_fan_seq_opts {
    uint64_t seed;            /* every rank of the job passes the same seed          */
    int32_t  check;           /* 1: checksum + poison every received block           */
    int32_t  flags;           /* 0, MPX_XFER_STREAM or MPX_FAN_LL                    */
    uint32_t timeout_ms;      /* as mpx_fan_opts                                     */
    int32_t  nwg;             /* as mpx_fan_opts                                     */
    const uint64_t *expect;   /* check = 1: [npeers * iters], expect[k * iters + i] =
                                 mpx_checksum value of P(seed, peers[k], my_rank, i,
                                 block_len); NULL: the library computes them on the
                                 CPU before the launch                               */
} mpx_fan_seq_opts;
int mpx_xfer_fan_seq(mpx_ctx *ctx, int my_rank, int npeers, const int *peers, int iters,
                     void *tx, void *rx, int block_len, size_t stride,
                     const mpx_fan_seq_opts *opts, mpx_timing *t, mpx_fan_link *links);

#endif /* MPX_FAN_SEQ_H */
