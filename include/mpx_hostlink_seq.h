/* mpx_hostlink_seq.h - sequenced payloads on the host link: the ping-pong and
   unidir loops between a GPU rank and a CPU endpoint with a payload of its
   own in every iteration.  Part of the C-ABI of include/mpx.h, which includes
   this file inside its extern "C" block: include "mpx.h", not this file. */
#ifndef MPX_HOSTLINK_SEQ_H
#define MPX_HOSTLINK_SEQ_H
#ifndef MPX_H
#error "include mpx.h: it includes mpx_hostlink_seq.h where the types it needs are declared"
#endif

/* ---- sequenced payloads on the host link ------------------------------------- */
/* mpx_xfer_hostlink / mpx_host_xfer re-send the same tx in every iteration, as
   the reference does, so a credit that is seen one push early or a pull that
   is served a stale copy leaves the bytes it would have left anyway.  The two
   calls below run the same loops with the payload of include/mpx_seq.h,
       P(seed, s, d, i, n) = the first n bytes mpx_fill(MPX_FILL_SPLITMIX,
                             mpx_pattern_key(seed, s, d, i)) writes,
   as the message rank s sends to rank d in iteration i: n = buff_len, or 1 for
   the unidir ack (byte 0 of the acking side's pattern of that iteration).
   Ranks are the context's rank numbers, the endpoint's included.
     GPU -> CPU: the pushing kernel generates the bytes in registers; the GPU
   rank's tx is neither read nor written.
     CPU -> GPU: an LL send packs its granules from generated words and does
   not touch the endpoint's tx.  A bulk send is a pull across the link, so the
   endpoint WRITES P(seed, host, gpu, i, n) into its tx[0 : n) before it says
   "tx holds message k" - strictly after every chunk's credit of the send
   before, which is the order the blocking loops always had.  After a call
   whose sends were bulk, the endpoint's tx[0 : n) holds payload iters - 1;
   bytes past n are untouched.  The GPU's loads of iteration i must therefore
   fetch iteration i's bytes across the link: a check failure here is a stale
   pull or an early credit.
     After any completed call, checked or not, rx[0 : recv_len) of either side
   holds P(seed, peer, me, iters - 1, recv_len).
     Everything else is the ordinary host-link call's: the modes (ping-pong
   and unidir only), groups, argument checks, the LL / bulk choice
   (mpx_hostlink_ll_max, MPX_HOSTLINK_LL), the width (nwg, MPX_HOSTLINK_WG),
   the receive-posted handshake, flags, credits, mpx_timing (protocol 11 or
   12), mpx_last_phases, the link counters, deadlines and MPX_ERR_TIMEOUT.  So
   sequenced and ordinary host-link calls may alternate on one link, and with
   pair, fan and full-duplex calls; and the two sides of a call need not
   agree: if only one side makes the sequenced call both calls complete, and
   the sequenced side receives the peer's tx bytes - which an unchecked call
   cannot notice.
     opts is mpx_seq_opts (mpx_seq.h): seed, check, timeout_ms, nwg, expect.
   Check mode: payload i is compared with expect[i], so check_iters = iters
   and check_failures counts the iterations that differ; recv_digest is the sum
   of the finished checksums.  expect == NULL: the library computes the
   expectations on the CPU before the timed part of the call; refused when
   iters * recv_len exceeds MPX_SEQ_AUTO_MAX.
     Statuses, all decided before any GPU work:
       whatever mpx_xfer_hostlink / mpx_host_xfer refuse (MPX_ERR_UNSUPPORTED
         for MPX_MODE_NONBLOCKING or another engine, MPX_ERR_INVALID for ranks
         that are not a local GPU rank and a host endpoint, ...)
       MPX_ERR_INVALID   NULL ctx / opts / t; any flags bit at all (no tx is
                         read, so MPX_XFER_NOSTAGE means nothing, and
                         MPX_XFER_STREAM is refused on the host link already);
                         expect == NULL above MPX_SEQ_AUTO_MAX
       MPX_ERR_STATE     a GPU rank that holds an armed call, or either end
                         after a call that timed out
     Afterwards: MPX_ERR_TIMEOUT, MPX_ERR_CHECK.
     A sequenced call is never traced: with mpx_hostlink_lat_enable on, it
   runs untraced and leaves the recorder's blocks as they were.
     mpx_xfer_seq keeps refusing a host endpoint, and the full-duplex loop
   (mpx_hostlink_duplex.h) stays unsequenced: its 256-slot window keeps sends
   in flight while the next one would have to overwrite tx.
     The ABI version is unchanged: callers detect the feature by symbol. */
int mpx_xfer_hostlink_seq(mpx_ctx *ctx, int mode, int my_group, int my_rank, int host_rank, int iters, void *tx, void *rx,
                          int buff_len, const mpx_seq_opts *opts, mpx_timing *t);
int mpx_host_xfer_seq(mpx_ctx *ctx, int mode, int my_group, int host_rank, int peer_rank, int iters, int buff_len,
                      const mpx_seq_opts *opts, mpx_timing *t);

#endif /* MPX_HOSTLINK_SEQ_H */
