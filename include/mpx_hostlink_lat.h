/* mpx_hostlink_lat.h - the host-link recorder of libmpx: the per-iteration
   latency distribution of the host link's ping-pong and unidir loops, recorded
   on the GPU end and on the CPU end, each with its own clock.  Part of the
   C-ABI of include/mpx.h, which includes this file inside its extern "C"
   block: include "mpx.h", not this file. */
#ifndef MPX_HOSTLINK_LAT_H
#define MPX_HOSTLINK_LAT_H
#ifndef MPX_H
#error "include mpx.h: it includes mpx_hostlink_lat.h where the types it needs are declared"
#endif

/* ---- host link: per-iteration latency distribution, on both ends ----------- */
/* What mpx_lat_* is to a rank's pair calls and mpx_fan_lat_* to the links of
   its LL fan calls, for the host link (mpx_hostlink.h) - the first recorder
   whose iterations cross a link.  `rank` is either an attached local GPU rank
   or a host endpoint; each end is enabled on its own.
     - Scope.  While a rank's host-link recorder is enabled, every
       mpx_xfer_hostlink call (a GPU rank) or mpx_host_xfer call (an endpoint)
       of that rank records the time of each of its iterations into a block
       keyed by the PEER'S RANK: a GPU rank may have several endpoints and an
       endpoint several GPU ranks.  A block accumulates over every traced call
       with that peer until mpx_hostlink_lat_reset; `calls` counts them.  A
       peer never used reads all zeros (with tick_s set), not an error.
     - Format.  The block is mpx_lat as it is: the same fields, the same 464
       buckets; mpx_lat_bucket, _bucket_floor and _quantile apply unchanged.
       THE TWO ENDS' TICKS DIFFER: on a GPU rank tick_s = 1e-8 (the kernel's
       clock, the clock of mpx_phases); on an endpoint tick_s = 1e-9
       (CLOCK_MONOTONIC in nanoseconds, the clock the endpoint's deadlines
       use).  Multiply by tick_s before comparing the two.  On an endpoint a
       delta of 2^32 ns (4.3 s) or more clamps into the last bucket; min, max
       and sum stay exact.
     - Stamps, GPU rank (workgroup 0's lane 0): t[0] is the instant
       mpx_phases.first_iter_s counts from - the endpoint's post seen, on a
       side that pushes first, else the kernel's entry, so a side that
       receives first has the wait for a late endpoint in its first delta;
       t[i+1] at the bottom of iteration i.  d[0] = first_iter_s.
       Stamps, endpoint (the thread inside mpx_host_xfer): t[0] right before
       the loop - its post is stored and, on a side that sends first, the GPU
       rank's post was seen; t[i+1] when iteration i's last step has
       returned, check and poison included.
       d = t[i+1] - t[i]; sum_ticks telescopes to t[iters] - t[0].  A call with
       iters = 0 adds 1 to calls, sets last_iters = 0 and adds nothing else.
     - Tracing is local: it touches only the recording side's own memory and
       changes no byte on the link.  The two ends need not agree on it.
     - What is not traced: full-duplex calls (mpx_xfer_hostlink_duplex,
       mpx_host_xfer_duplex), pair calls and fan calls on an enabled rank run
       untraced and leave this recorder untouched (the rule of the
       non-blocking loop under mpx_lat_*).  A host-link call leaves mpx_lat_*
       and mpx_fan_lat_* untouched.  All three recorders may be enabled at
       once.
     - MPX_ERR_UNSUPPORTED: enable on an SDMA or RCCL context.
       MPX_ERR_INVALID: a NULL ctx or NULL out / stamps / n; a rank that is
       neither a local GPU rank nor a host endpoint; raw_cap outside
       [0, MPX_HOSTLINK_LAT_RAW_MAX]; peer out of range or equal to rank.
       MPX_ERR_STATE: any of the five on a GPU rank that holds an armed call;
       reset / get / raw on a rank that is not enabled.
     - The recorder never makes a transfer fail.  A call that fails (timeout,
       check) leaves the contents undefined until mpx_hostlink_lat_reset.
     - Threading: an endpoint's block is written by the thread inside
       mpx_host_xfer; the caller reads or resets it only between that
       endpoint's calls - the rule a GPU rank's block already has.
     - With the recorder off a call runs exactly what it ran before, on both
       ends: traced GPU calls run kernels of their own (k_hostlink_lat), the
       traced endpoint loop is an instantiation of its own.
   The ABI version is unchanged: callers detect the feature by symbol. */
#define MPX_HOSTLINK_LAT_RAW_MAX (1 << 16)   /* largest raw_cap mpx_hostlink_lat_enable accepts */
/* raw_cap: stamps kept per peer and call beyond t[0]; allocates nranks blocks
   (device memory on a GPU rank, ordinary host memory on an endpoint); resets */
int mpx_hostlink_lat_enable(mpx_ctx *ctx, int rank, int raw_cap);
int mpx_hostlink_lat_disable(mpx_ctx *ctx, int rank);
int mpx_hostlink_lat_reset(mpx_ctx *ctx, int rank);   /* every peer's block */
int mpx_hostlink_lat_get(mpx_ctx *ctx, int rank, int peer, mpx_lat *out);
/* link (rank, peer)'s stamps t[0 .. min(iters, raw_cap)] of the last traced
   call with that peer, at most `cap` of them; *n = how many were written */
int mpx_hostlink_lat_raw(mpx_ctx *ctx, int rank, int peer, uint64_t *stamps, int cap, int *n);

#endif /* MPX_HOSTLINK_LAT_H */
