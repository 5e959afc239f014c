/*
 * mpx_host.h — host-side logic of mpx_perf (pure C, no HIP): command line,
 * group/peer rule, all-pairs round schedule, CSV records and log files.
 * Built into libmpx_host.so (tested on CPU against tests/golden) and linked
 * into the mpx_perf executable.
 *
 * Reference: /root/reference/mpi_perf.c — every function cites its lines.
 */
#ifndef MPX_HOST_H
#define MPX_HOST_H

#include <stddef.h>
#include <stdio.h>

#define MPXH_MAX_HOST 128          /* MAX_HOST_SZ            mpi_perf.c:13  */
#define MPXH_DEF_BUF_SZ 456131     /* DEF_BUF_SZ             mpi_perf.c:14  */
#define MPXH_DEF_ITERS 10          /* DEF_ITERS              mpi_perf.c:15  */
#define MPXH_LOG_REFRESH_SEC 900   /* LOG_REFRESH_TIME_SEC   mpi_perf.c:16  */
#define MPXH_MAX_RANKS 64

/* struct options, mpi_perf.c:257-268, plus the MI355X-only settings.  The
   first nine fields keep the reference's meaning and defaults. */
typedef struct mpxh_options {
    int use_dotnet;                 /* -d */
    int iters;                      /* -i */
    int buff_sz;                    /* -b */
    int uni_dir;                    /* -u */
    int num_runs;                   /* -r  (-1 = forever)   */
    int ppn;                        /* -p */
    int nonblocking;                /* -x */
    char uuid[64];
    char logfolder[MPXH_MAX_HOST];  /* -l */
    /* not in the reference */
    char group1_hostfile[MPXH_MAX_HOST]; /* -f (a global in mpi_perf.c:254) */
    int group_size;                 /* -n (a global in mpi_perf.c:255) */
    int world;                      /* -w  ranks (mpirun -np);  0 = 2*ppn   */
    int engine;                     /* -e  0 kernel, 1 sdma, 2 rccl          */
    int all_pairs;                  /* -a  1 = circle-method rounds           */
    int check;                      /* -c  1 = checksum every payload, 2 = and
                                           seeded-pattern payloads            */
    int sweep_min, sweep_max;       /* -S  min:max  power-of-two size sweep   */
    int timeout_ms;                 /* -t  per-wait device timeout            */
    char gpus[256];                 /* -g  rank->GPU list "0,1,..."          */
    int arm;                        /* -A  1 (default) = arm each run's kernel
                                           before the barrier (mpx_xfer_arm) */
    int lat_cap;                    /* -L  raw_cap: record every iteration's
                                           latency (mpx_lat_*), lat-*.csv;
                                           -1 (default) = off                */
    int fan;                        /* -m  1 = every run is one fan exchange of
                                           every rank with all the others
                                           (mpx_xfer_fan); 2 = the same as a
                                           lock-step LL exchange (MPX_FAN_LL) */
    int arm_set;                    /* -A was given on the command line       */
    int fan_lat_cap;                /* -P  raw_cap: with -m 2, record every
                                           link's per-iteration exchange latency
                                           (mpx_fan_lat_*), lat-*.csv; -1
                                           (default) = off                    */
    int hostlink;                   /* -H  1|2: every rank is a GPU rank paired
                                           with a host endpoint of its own, rank
                                           world + r (mpx_xfer_hostlink /
                                           mpx_host_xfer); 1 = the GPU rank is
                                           group 1 (sends first), 2 = group 0 */
    int procs;                      /* set by the host before mpxh_validate: 1 =
                                           one process per rank (a launcher)  */
    int duplex;                     /* -X  1: with -H, every run is the
                                           full-duplex non-blocking loop across
                                           the host link
                                           (mpx_xfer_hostlink_duplex /
                                           mpx_host_xfer_duplex)              */
    int hostlink_lat_cap;           /* -T  raw_cap: with -H, record every
                                           iteration's latency on both ends of
                                           the host link (mpx_hostlink_lat_*),
                                           lat-*.csv; -1 (default) = off      */
    int fan_seq;                    /* -Q  1: with -m 1|2, every run is one
                                           sequenced fan call (mpx_xfer_fan_seq):
                                           a payload per (src, dst, iteration);
                                           a malformed value reads as -1      */
    int hostlink_seq;               /* -K  1: with -H 1|2 (not -X 1), every run
                                           is a sequenced host-link call on both
                                           ends (mpx_xfer_hostlink_seq /
                                           mpx_host_xfer_seq); a malformed value
                                           reads as -1                        */
} mpxh_options;

/* parse status */
enum {
    MPXH_PARSE_OK = 0,
    MPXH_PARSE_USAGE = 1,           /* unknown flag / -h: usage + abort      */
    MPXH_PARSE_BAD_VALUE = 2,       /* a value of a new flag is malformed    */
    MPXH_PARSE_CRASH = 3,           /* the reference dereferences a missing
                                       argument (Windows variant)           */
    MPXH_PARSE_BAD_DUPLEX = 4,      /* -X with a value other than 0 or 1     */
    MPXH_PARSE_BAD_HOSTLINK_LAT = 5 /* -T with a malformed raw_cap           */
};

/* defaults of main(), mpi_perf.c:388-392 (+ the new fields) */
void mpxh_defaults(mpxh_options *o);
/* parse_args, mpi_perf.c:273-339 (getopt ":f:n:d:p:i:b:u:h:r:l:x:" plus
   "w:e:a:c:S:t:g:A:L:m:P:H:X:T:Q:K:"); fills o->uuid with a fresh v4 UUID.  Resets getopt. */
int mpxh_parse_args(mpxh_options *o, int argc, char **argv);
/* print_usage, mpi_perf.c:20-32 (the reference's text, then the new flags) */
void mpxh_print_usage(FILE *f);
/* engine name <-> id */
int mpxh_engine_from_name(const char *s);
const char *mpxh_engine_name(int e);

/* -m 1: blocks of a fan run lie `stride` apart in tx and rx: -b rounded up to
   4096 (the alignment mpx_alloc gives a buffer) */
#define MPXH_FAN_ALIGN 4096
/* -m 2: the largest -b (MPX_FAN_LL_MAX, include/mpx.h) */
#define MPXH_FAN_LL_MAX 4096
/* -c 3: the most bytes of expected payloads per run, -i x -b (MPX_SEQ_AUTO_MAX,
   include/mpx_seq.h), and the run's seed: the same on both sides of a link */
#define MPXH_SEQ_AUTO_MAX (1ull << 28)
#define MPXH_SEQ_RUN_SEED(pattern_seed, run_idx) \
    ((unsigned long long)(pattern_seed) + (unsigned long long)(run_idx) * 0x9E3779B97F4A7C15ull)
/* -H: a rank's host endpoint is rank world + r of the same context */
#define MPXH_HOSTLINK_MAX_WORLD (MPXH_MAX_RANKS / 2)
size_t mpxh_fan_stride(int buff_len);
/* bytes of a fan run's tx (and rx): world blocks; 0 if that exceeds the
   largest length a rank can attach (2^31 - 1) or an argument is negative */
size_t mpxh_fan_bytes(int world, int buff_len);
/* the peers of `rank` in a fan run, in rank order: everyone else.  Returns
   their number (world - 1). */
int mpxh_fan_peers(int world, int rank, int *peers);

/* validate -L against -x / -e (the recorder traces the kernel engine's
   blocking loops only) and -m 1 against -a 1, an explicit -A 1, -L, -e, -d 1
   and a -b too large for world blocks (-m 2: the same, and a -b above
   MPXH_FAN_LL_MAX), and -P without -m 2; -H against -x 1, -a 1, -m, an
   explicit -A 1, -L, -d 1, -e sdma|rccl, processes mode and -w above
   MPXH_HOSTLINK_MAX_WORLD, and -T without -H or with -X 1; -c 3 against
   -e sdma|rccl, -m, -H, an explicit -A 1, -L and -i x -b above
   MPXH_SEQ_AUTO_MAX; -Q against a value other than 0 or 1, a run without
   -m, -c 2, -P and, with -c 1, (world - 1) x -i x -b above
   MPXH_SEQ_AUTO_MAX (-c 3 with -m keeps its own refusal, which comes
   first); -K against a value other than 0 or 1, a run without -H, -X 1,
   -T, -c 2|3 and, with -c 1, -i x -b above MPXH_SEQ_AUTO_MAX; then group_size, mpi_perf.c:399-403 (with -H the
   job is the 2 * world ranks: the GPU ranks and their endpoints).
   Returns:
   0 ok, 1 invalid (message printed, caller aborts), 2 the reference divides
   by zero here (ppn == 0 in bidirectional mode): the caller raises SIGFPE. */
int mpxh_validate(const mpxh_options *o, int world, FILE *err);
/* read the -f file with fgets into group_size lines of MAX_HOST bytes,
   mpi_perf.c:405-418.  Returns a calloc'd block or NULL (cannot open). */
char *mpxh_read_group1(const char *path, int group_size);

/* strnicmp, mpi_perf.c:34-53 */
int mpxh_strnicmp(const char *s1, const char *s2, size_t n);
/* membership, mpi_perf.c:437-444 */
int mpxh_in_group1(const char *name, const char *lines, int group_size);
/* Comm_split + peer, mpi_perf.c:447-450, :225-233 */
void mpxh_pairing(int world, const int *group, int *group_rank, int *group_size, int *peer);

/* Virtual processor name of rank r: "<node>-<r / ppn>" (ppn ranks per
   virtual host, as --map-by ppr:ppn:node places them); MPX_PROCESSOR_NAMES
   ("a,a,b,b") overrides.  Writes into out[MPXH_MAX_HOST]. */
void mpxh_processor_name(char *out, const char *node, int rank, int ppn, const char *override_list);

/* circle-method 1-factorisation: round r of n ranks (even
   n >= 2) -> pairs[k] = {g1, g0}, k < n/2.  Returns n/2 or -1. */
int mpxh_round_pairs(int n, int r, int (*pairs)[2]);
/* role of `rank` in round r: *group (1/0) and *peer.  Returns 0 or -1. */
int mpxh_round_role(int n, int r, int rank, int *group, int *peer);

/* parse "0,1,2" into devs[] (max n); returns count or -1 */
int mpxh_parse_gpu_list(const char *s, int *devs, int n);

/* time strings, getformatted_time mpi_perf.c:341-353 */
void mpxh_format_time(char *buf, size_t cap, int for_kusto);
/* lat-*.csv (-L): header, and one line per recorded run; times in us
   (-m 2 -P: one line per link and recorded run, Mode = 10) */
#define MPXH_FAN_LAT_RAW_MAX (1 << 16) /* MPX_FAN_LAT_RAW_MAX, include/mpx_fan_lat.h */
#define MPXH_FAN_LAT_MODE 10           /* the LL fan call's protocol number  */
/* -H -T: one line per end and recorded run, Mode = the call's protocol number (11 LL, 12 bulk) */
#define MPXH_HOSTLINK_LAT_RAW_MAX (1 << 16) /* MPX_HOSTLINK_LAT_RAW_MAX, include/mpx_hostlink_lat.h */
#define MPXH_LAT_HEADER                                                                                   \
    "Timestamp,JobId,Rank,PeerRank,Mode,BufferSize,NumOfBuffers,RunId,Count,MinUs,P50Us,P90Us,P99Us,P999Us," \
    "MaxUs,MeanUs,MaxIter\n"
int mpxh_format_lat(char *out, size_t cap, const char *timestamp, const char *uuid, int rank, int peer, int mode,
                    int buff_len, int iters, long long run_idx, unsigned long long count, const double us[7],
                    unsigned long long max_iter);
/* record line, mpi_perf.c:550-554 */
int mpxh_format_record(char *out, size_t cap, const char *timestamp, const char *uuid, int world_rank,
                       int world_size, int ppn, const char *local_ip, const char *remote_ip, int buff_len,
                       int iters, double my_time_s, long long run_idx);
/* log file name, mpi_perf.c:494 */
int mpxh_log_name(char *out, size_t cap, const char *logfolder, const char *uuid, int world_rank,
                  const char *file_time);
/* REPORT_BANDWIDTH line, mpi_perf.c:535-541 */
int mpxh_format_bandwidth(char *out, size_t cap, int world_rank, long long run_idx, int buff_len, int iters,
                          int uni_dir, double my_time_s);
/* rank-0 summary, mpi_perf.c:564-568 */
int mpxh_format_summary(char *out, size_t cap, long long run_idx, double total_s, double min_s, double max_s,
                        double sum_s, int world);
/* INFO line, mpi_perf.c:460-461 */
int mpxh_format_info(char *out, size_t cap, const char *name, int rank, int world, int group, int group_size,
                     int group_rank, int peer, const char *my_ip, const char *peer_name, const char *peer_ip);
/* .NET launcher lines, mpi_perf.c:147-168 (printed, never executed) */
int mpxh_format_dotnet(char *out, size_t cap, int my_group, int my_rank, int peer_rank, const char *peer_ip,
                       const char *my_ip, int buff_len, int iters, int ppn);
/* v4 UUID (libuuid's uuid_generate + uuid_unparse, mpi_perf.c:335-337) */
void mpxh_uuid(char out[37]);
/* IPv4 of a host name: last AF_INET result like get_ipaddress,
   mpi_perf.c:171-198.  Returns 0 ok, -1 lookup failed. */
int mpxh_ipv4(const char *host, char *out, size_t cap);

/* ---- the Windows / MS-MPI variant, windows/mpi-perf.cpp ----------------- */
/* 7-character job id (generate_uuid's sizeof(char *) truncation, :175-184) */
void mpxh_uuid_windows(char out[64]);
/* positional parse_args, :187-197, over main's defaults :226-230 */
int mpxh_parse_args_windows(mpxh_options *o, int argc, char **argv);
/* group-1 address lines with the newline cut off, :249-261 */
char *mpxh_read_group1_windows(const char *path, int group_size);
/* whole-address case-insensitive membership, :283-289 */
int mpxh_in_group1_windows(const char *addr, const char *lines, int group_size);
/* Comm_split + last-match peer, :114-133, :292-295 */
void mpxh_pairing_windows(int world, const int *group, int *group_rank, int *group_size, int *peer);

#endif
