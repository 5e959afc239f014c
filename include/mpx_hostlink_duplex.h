/* mpx_hostlink_duplex.h - the host link's full-duplex loop: the reference's
   non-blocking loop between a GPU rank and a CPU endpoint, both directions of
   the PCIe link loaded at once.  Part of the C-ABI of include/mpx.h, which
   includes this file inside its extern "C" block, after mpx_hostlink.h:
   include "mpx.h", not this file. */
#ifndef MPX_HOSTLINK_DUPLEX_H
#define MPX_HOSTLINK_DUPLEX_H
#ifndef MPX_HOSTLINK_H
#error "include mpx.h: it includes mpx_hostlink_duplex.h after mpx_hostlink.h, whose endpoints it uses"
#endif

/* ---- host link: the non-blocking loop, full duplex -------------------------- */
/* The two calls below run do_mpi_benchmark_nonblocking (mpi_perf.c:85-125)
   between an attached local GPU rank and a host endpoint (mpx_host_attach) of
   the same context.  There is no mode and no group argument: both sides run
   the same loop, as mpx_xfer_ex says of MPX_MODE_NONBLOCKING ("both sides
   alike").  mpx_xfer_hostlink and mpx_host_xfer go on refusing that mode; the
   loop lives behind these two names, and callers detect it by symbol (the ABI
   version is unchanged).
     The loop.  Per iteration one B-byte send and one B-byte receive, neither
   waited for.  At window slot 255 Waitall covers the sends and receives of
   slots 0..254; after the loop Waitall(inflight) runs.  So recv_done =
   iters - iters / 256: slot 255 of each full window is never waited for.
   bytes = 2 * B * iters; launches is 1 on the GPU side and 0 on the CPU side;
   protocol = 13; nwg is the PER-DIRECTION width.  There is no LL path (the
   pair loops have none in this mode either): an 8-byte or a 0-byte message
   goes through the bulk form at width 1.
     Directions.  GPU -> CPU: the bulk push into the endpoint's rx; the drain
   and in.flag[w] follow the non-blocking loop's publish schedule — every
   MPX_NB_PUBLISH pushes (default 16), at window slot 254 and at the last
   push.  MPX_XFER_NOSTAGE and LDS staging work as in mpx_xfer_hostlink.
   CPU -> GPU: "Isend" i is one release store of out.ready = tx_seq0 + i + 1;
   the GPU's workgroups pull their chunks of the endpoint's tx, and
   in.credit[w] and the landed count are published every MPX_NB_PUBLISH
   receives, at window slot 254 (the last receive a flush waits for) and at
   the last.  The kernel runs a split grid of 2 * nwg workgroups: nwg push and
   nwg pull, and the two halves meet only at window flushes and at the end.
     Buffer reuse.  Each side returns only after every one of its iters sends
   is complete: the CPU side waits for every credit, the GPU's pushes are
   drained (and the CPU side has then seen every flag: its rx is quiet too).
   Counting follows the reference's rule all the same.  Neither end's tx may
   change during a call.
     Ordering.  The receives-posted handshake is mpx_xfer_hostlink's: no byte
   of call k lands in the endpoint's rx before the endpoint has entered call
   k; the GPU rank's rx is only ever written by its own kernel.  Link
   counters, call number and token move as for a non-blocking pair call:
   mpx_link_counters shows +iters, +iters, +1 on either end.
     Check mode (opts.check, expect_checksum) checksums EVERY payload of both
   directions, the ones the reference leaves pending too: check_iters = iters.
   recv_digest sums the counted receives only (j % 256 != 255).  Every payload
   but the last is poisoned.  The GPU checks its pulled chunk as it lands.  The
   CPU receives into one rx, so the GPU -> CPU direction is paced: push i + 1
   is stored only after the CPU has checked and poisoned payload i and said so
   in the endpoint's out.credit row, and every push is published.  Check mode
   is not a bandwidth mode.  Every CPU wait — a window flush, the end —
   services landed receives while it waits, so neither side can starve the
   other.
     Waits.  All are bounded: the kernel's by opts.timeout_ms on its own
   clock, the CPU's by the same opts.timeout_ms against CLOCK_MONOTONIC (0 =
   10 s).  A timeout returns MPX_ERR_TIMEOUT and that side is then broken
   (MPX_ERR_STATE).
     Statuses, all decided before any GPU work or wait, with
   mpx_xfer_hostlink's rules:
       MPX_ERR_UNSUPPORTED  an SDMA or RCCL context
       MPX_ERR_INVALID      NULL arguments; bad ranks or buffers; buff_len
                            above either attached length; any opts.flags bit
                            other than MPX_XFER_NOSTAGE; a per-direction width
                            above 128 (the split grid would exceed 256
                            workgroups)
       MPX_ERR_STATE        an armed or a broken rank
     Afterwards: MPX_ERR_TIMEOUT, MPX_ERR_CHECK.
     Width: opts.nwg, else MPX_HOSTLINK_WG, else one workgroup per 32 KiB up
   to 16 PER DIRECTION, then at least 1 KiB per workgroup — mpx_xfer_hostlink's
   rule, so both ends agree.
     The call is never traced by mpx_lat_* and cannot be armed;
   mpx_last_phases works for the GPU side.  MPX_TEST=skip_push=k loses the
   k-th B-byte payload of EACH direction (both carry payloads here): the GPU
   skips the stores of push k (its flags still come) and the loads of pull k
   (its credit still comes). */

/* GPU side: my_rank is an attached local GPU rank (tx / rx its attached
   buffers), host_rank a host endpoint of the same context */
int mpx_xfer_hostlink_duplex(mpx_ctx *ctx, int my_rank, int host_rank, int iters, void *tx, void *rx,
                             int buff_len, const mpx_xfer_opts *opts, mpx_timing *t);
/* CPU side, on the calling thread (peer_rank: the GPU rank) */
int mpx_host_xfer_duplex(mpx_ctx *ctx, int host_rank, int peer_rank, int iters, int buff_len,
                         const mpx_xfer_opts *opts, mpx_timing *t);

#endif /* MPX_HOSTLINK_DUPLEX_H */
