/* mpx_fan_lat.h - the link recorder of libmpx: the per-link latency
   distribution of the lock-step LL fan exchange (MPX_FAN_LL).  Part of the
   C-ABI of include/mpx.h, which includes this file where mpx_lat is declared
   (inside its extern "C" block): include "mpx.h", not this file. */
#ifndef MPX_FAN_LAT_H
#define MPX_FAN_LAT_H
#ifndef MPX_H
#error "include mpx.h: it includes mpx_fan_lat.h where the types it needs are declared"
#endif

/* ---- per-link latency distribution of the lock-step LL fan exchange ------- */
/* The link recorder: what mpx_lat_* is to a rank's pair calls, per LINK of a
   rank's MPX_FAN_LL calls.  While a rank's link recorder is enabled, every
   mpx_xfer_fan call of that rank with MPX_FAN_LL records, for each of its
   links, the time of each iteration of that link's lock-step loop, into a
   block of that link's own (mpx_lat as it is: the same fields, tick_s = 1e-8,
   the same histogram; mpx_lat_bucket, _bucket_floor and _quantile apply).
     - Stamps (the kernel's clock, read by the link's own workgroup): t[0]
       right after the workgroup has seen the peer's post (once per call,
       before the first push); t[i+1] at the bottom of iteration i: the peer's
       push i has arrived and its unpack stores are issued and, in check
       mode, the block is checked.  d = t[i+1] - t[i] is one full exchange
       with that peer; sum_ticks telescopes to t[iters] - t[0].  A call with
       iters = 0 adds 1 to calls, sets last_iters = 0 and adds nothing else.
     - Blocks are keyed by the PEER'S RANK, not by its position in peers[]: a
       rank may list its peers in any order and with a different set per
       call.  Link (rank, peer) accumulates over every traced call that listed
       `peer`, until mpx_fan_lat_reset; `calls` counts those calls.  A peer
       never listed reads all zeros (with tick_s set), not an error.
     - Bulk fan calls (no MPX_FAN_LL) and pair calls on an enabled rank run
       untraced and leave the link recorder untouched; an LL fan call leaves
       the rank recorder (mpx_lat_*) untouched.  The two recorders are
       independent; both may be enabled at once.
     - Tracing touches only this rank's memory and changes no byte on the
       link: the two ends of a link need not agree on it.
     - MPX_ERR_UNSUPPORTED: enable on the SDMA / RCCL engines.
       MPX_ERR_INVALID: a NULL ctx or NULL out / stamps / n, a rank that is
       not local, raw_cap outside [0, MPX_FAN_LAT_RAW_MAX], peer out of range
       or equal to rank.  MPX_ERR_STATE: any of the five on a rank that holds
       an armed call; reset / get / raw on a rank that is not enabled.
     - The recorder never makes a transfer fail.  A call that fails (timeout,
       check) leaves the contents undefined until mpx_fan_lat_reset.
     - With the recorder off an LL fan call runs the kernels it ran before:
       traced calls run instantiations of their own (k_xfer_fan_ll<., true>).
   The ABI version is unchanged: callers detect the feature by symbol. */
#define MPX_FAN_LAT_RAW_MAX (1 << 16)   /* largest raw_cap mpx_fan_lat_enable accepts */
/* raw_cap: stamps kept per link and call beyond t[0]; allocates nranks blocks
   (at 64 ranks and 2^16 about 32 MiB, hence the smaller limit); resets */
int mpx_fan_lat_enable(mpx_ctx *ctx, int rank, int raw_cap);
int mpx_fan_lat_disable(mpx_ctx *ctx, int rank);
int mpx_fan_lat_reset(mpx_ctx *ctx, int rank);   /* every peer's block */
int mpx_fan_lat_get(mpx_ctx *ctx, int rank, int peer, mpx_lat *out);
/* link (rank, peer)'s stamps t[0 .. min(iters, raw_cap)] of the last traced
   call that listed peer, at most `cap` of them; *n = how many were written */
int mpx_fan_lat_raw(mpx_ctx *ctx, int rank, int peer, uint64_t *stamps, int cap, int *n);

#endif /* MPX_FAN_LAT_H */
