/* mpx_hostlink.h - the host link of libmpx: the pair loops between a GPU rank
   and a CPU endpoint, across the PCIe link between the GPU and the host.
   Part of the C-ABI of include/mpx.h, which includes this file inside its
   extern "C" block: include "mpx.h", not this file. */
#ifndef MPX_HOSTLINK_H
#define MPX_HOSTLINK_H
#ifndef MPX_H
#error "include mpx.h: it includes mpx_hostlink.h where the types it needs are declared"
#endif

/* ---- host link: a GPU rank and a CPU endpoint ------------------------------ */
/* A HOST ENDPOINT is a rank number of the context whose tx, rx and mailbox
   live in pinned host memory and whose side of the loop runs on a CPU thread.
   It is neither "local" nor "imported": mpx_xfer_ex, mpx_xfer_fan,
   mpx_xfer_arm, mpx_rank_export, mpx_lat_* and every other entry point refuse
   it exactly as they refuse a rank that was never attached.
     The two calls below run the reference's ping-pong loop (mpi_perf.c:66-83)
   or its unidirectional loop (:127-145, with its 1-byte ack) with the meaning
   mpx_xfer_ex gives them between two GPU ranks: the two sides pass opposite
   my_group values and group 1 sends first; each side returns when its own
   side of the loop is complete; recv_done counts every receive as the
   reference's loop completes them; bytes is the a9 formula.  Check mode
   (opts.check, expect_checksum, expect_ack) checksums every received payload
   and poisons every payload but the last, on whichever side receives — the
   CPU side with mpx_host_checksum and the kernels' poison.
     A host endpoint cannot write device memory: every word and byte that
   crosses the link lives in pinned host memory (hipHostMalloc, mapped,
   coherent, portable) and the GPU does all the moving.  GPU -> CPU: LL
   granules up to the LL threshold, above it the bulk push into the
   endpoint's rx (payload stores, per-workgroup drain, flag).  CPU -> GPU: LL
   granules the GPU's workgroup 0 polls across the link, above the threshold
   "tx holds message k" and the GPU's workgroups load their chunks of the
   endpoint's tx themselves.  A payload of call k lands only after its
   receiver has entered call k.  Every wait is bounded on both sides:
   the GPU's by opts.timeout_ms on the kernel's clock, the CPU's by the same
   opts.timeout_ms against CLOCK_MONOTONIC (0 = 10 s).
     Statuses, all decided before any GPU work or wait:
       MPX_ERR_UNSUPPORTED  an SDMA or RCCL context; MPX_MODE_NONBLOCKING
                            (the full-duplex loop has entry points of its
                            own: mpx_hostlink_duplex.h)
       MPX_ERR_INVALID      NULL arguments; a host_rank that is not a host
                            endpoint or a GPU rank that is not an attached
                            local rank; tx / rx other than the GPU rank's
                            attached buffers; buff_len above either attached
                            length; any opts.flags bit other than
                            MPX_XFER_NOSTAGE (MPX_XFER_STREAM: nontemporal
                            stores without system scope do not show in host
                            memory; MPX_XFER_PULL: the direction of each
                            transfer is fixed)
       MPX_ERR_STATE        a GPU rank that holds an armed call; a rank, GPU
                            or host endpoint, that timed out before
     Afterwards: MPX_ERR_TIMEOUT (that side is broken: its later calls return
   MPX_ERR_STATE), MPX_ERR_CHECK.
     Width: opts.nwg, else the environment's MPX_HOSTLINK_WG, else one
   workgroup per 32 KiB up to 16 (measured: DESIGN.md §5 "Host link"); then at
   least 1 KiB per workgroup.  Both ends compute it from the same inputs.
     Timing: protocol 11 = host link with LL granules, 12 = host link bulk.
   The GPU side fills mpx_timing as a pair call does (launches = 1), and
   mpx_last_phases works for it.  The CPU side reports wall_s from
   CLOCK_MONOTONIC, device_s = 0, launches = 0 and the link's nwg.
     mpx_link_counters accepts either end as my_rank (out[3] = 0 for a host
   endpoint); the counters move as for a pair call.  The test-only
   mpx_test_advance_link accepts either end too (a host endpoint with
   token_by = 0 only; both ends of a link must be advanced alike).  Host-link calls are
   never traced by the latency recorder (mpx_lat_*), like non-blocking calls,
   and cannot be armed.  MPX_TEST=skip_push=k loses the k-th B-byte payload of
   a sending side (never an LL ack).  The host link has a recorder of its own,
   on both ends: mpx_hostlink_lat.h.
   The ABI version is unchanged: callers detect the feature by symbol. */

/* Make `rank` a host endpoint with tx and rx of len bytes each (len = 0: 16
   zeroed bytes each, as mpx_alloc) and its mailbox.  Kernel engine only
   (MPX_ERR_UNSUPPORTED); MPX_ERR_INVALID for a NULL ctx, a rank out of range
   or len above 2^31 - 1; MPX_ERR_STATE for a rank already registered.  The
   memory is freed by mpx_finalize. */
int mpx_host_attach(mpx_ctx *ctx, int rank, size_t len);
/* the endpoint's tx and rx as CPU pointers, len bytes each (either may be NULL) */
int mpx_host_buffers(mpx_ctx *ctx, int rank, void **tx, void **rx);
/* GPU side: my_rank is an attached local GPU rank (tx / rx its attached
   buffers), host_rank a host endpoint of the same context */
int mpx_xfer_hostlink(mpx_ctx *ctx, int mode, int my_group, int my_rank, int host_rank, int iters,
                      void *tx, void *rx, int buff_len, const mpx_xfer_opts *opts, mpx_timing *t);
/* CPU side: runs the endpoint's side of the same loop on the calling thread
   (peer_rank: the GPU rank) */
int mpx_host_xfer(mpx_ctx *ctx, int mode, int my_group, int host_rank, int peer_rank, int iters,
                  int buff_len, const mpx_xfer_opts *opts, mpx_timing *t);
/* mpx_checksum's value, computed on the CPU; any alignment; no GPU, no ctx */
int mpx_host_checksum(const void *p, size_t n, uint64_t *out);
/* the LL threshold in force: the environment's MPX_HOSTLINK_LL (0...8192),
   else the default (256, measured: DESIGN.md §5 "Host link"); pure host, read
   at every call */
int mpx_hostlink_ll_max(void);

#endif /* MPX_HOSTLINK_H */
