/*
 * mosrx.h — C ABI of the MI355X receive-path classifier for mOS.
 *
 * One call classifies a batch of received Ethernet frames on a gfx950 GPU and
 * emits one 16-byte result record per frame.  The per-frame transform is the
 * part of mOS's software receive path that runs before the stateful flow
 * engine:
 *
 *   ProcessPacket          core/src/eth_in.c:27-87      (ethertype dispatch)
 *   ProcessInIPv4Packet    core/src/ip_in.c:30-101      (IPv4 checks)
 *   ip_fast_csum           core/src/include/ip_in.h:10-38
 *   ProcessInTCPPacket     core/src/tcp.c:408-445       (prefix up to FindStream)
 *   FillPacketContextTCPInfo core/src/tcp.c:258-270
 *   TCPCalcChecksum        core/src/tcp_util.c:157-190
 *   GetRSSHash/BuildKeyCache core/src/util.c:27-99     (Toeplitz RSS)
 *   GetRSSCPUCore          core/src/util.c:114-131     (queue map)
 *
 * The verdict in each record is bit-identical to ProcessPacket()'s return value
 * (1 / 0 / -1) for the same frame and the same stack state (num_msp, num_esp,
 * forward); `reason` distinguishes the causes that share a return value.
 *
 * Conventions (mirroring the reference's io_module_func, io_module.h:63-78):
 *   - every function returns 0 on success or a negative errno value;
 *   - the caller owns every buffer; the library never frees caller memory;
 *   - one mosrx_ctx per host thread (mOS runs one mTCP thread per core, and
 *     all io_module calls for a context come from that thread, core.c:1282-1349).
 *
 * No HIP, torch or C++ types appear in this header: streams are passed as
 * `void *` (a hipStream_t), device buffers as plain pointers.
 */
#ifndef MOSRX_H
#define MOSRX_H

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#else   /* compiled by hipRTC for a fused BPF kernel (csrc/bpf_jit.c): no libc headers there */
typedef unsigned char uint8_t;
typedef signed char int8_t;
typedef unsigned short uint16_t;
typedef unsigned int uint32_t;
typedef int int32_t;
typedef unsigned long long uint64_t;
typedef long long int64_t;
typedef unsigned long size_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MOSRX_ABI_VERSION 3

/* ---- per-frame result record (16 bytes) -------------------- */

/* reason codes */
enum {
	MOSRX_R_TCP_OK        = 0,  /* TCP segment passed every check        -> 1  (tcp.c:445)      */
	MOSRX_R_ARP           = 1,  /* ARP ethertype (RUN_ARP) or forwarded  -> 1  (eth_in.c:63-66) */
	MOSRX_R_NON_IPV4      = 2,  /* other ethertype: -1, or 1 if forward && num_msp (eth_in.c:62-77) */
	MOSRX_R_IP_SHORT      = 3,  /* tot_len < 20                          -> -1 (ip_in.c:42-45)  */
	MOSRX_R_IP_BADVER     = 4,  /* version != 4                          -> 0  (ip_in.c:47-51)  */
	MOSRX_R_NOVERIFY_PASS = 5,  /* num_msp == 0 && num_esp == 0          -> 1  (ip_in.c:67-72)  */
	MOSRX_R_IP_BADCSUM    = 6,  /* ip_fast_csum != 0                     -> -1 (ip_in.c:74-77)  */
	MOSRX_R_NOT_TCP       = 7,  /* protocol != TCP                       -> 0  (ip_in.c:82-93)  */
	MOSRX_R_TCP_SHORT     = 8,  /* ip_len < (ihl + doff) * 4             -> -1 (tcp.c:429-430)  */
	MOSRX_R_TCP_BADCSUM   = 9,  /* TCPCalcChecksum != 0                  -> -1 (tcp.c:432-444)  */
	MOSRX_R_TRUNCATED     = 10, /* build-only: a byte the reference reads lies past caplen -> -1 */
	MOSRX_R_TCP_LEN_OK    = 11, /* skip_tcp_csum mode: length check passed -> 1                 */
	MOSRX_R_ICMP_LOCAL    = 12, /* ICMP to a local address: ProcessICMPPacket -> 1 (ip_in.c:83-85, icmp.c:193-227) */
	MOSRX_R_COUNT         = 13
};

typedef struct mosrx_result {
	uint32_t rss;         /* GetRSSHash(ntohl(saddr), ntohl(daddr), ntohs(sport), ntohs(dport)); ports 0 if not TCP */
	uint16_t ip_csum;     /* raw ip_fast_csum() value (0 == valid); 0 if not computed */
	uint16_t tcp_csum;    /* raw TCPCalcChecksum() value (0 == valid); 0 if not computed */
	uint16_t payloadlen;  /* pkt_info.payloadlen (tcp.c:262, u16 arithmetic, may wrap) */
	uint8_t  payload_off; /* 14 + ihl*4 + doff*4 (<= 134); 0 if not TCP */
	int8_t   verdict;     /* ProcessPacket() return value: 1, 0 or -1 */
	uint8_t  reason;      /* MOSRX_R_* */
	uint8_t  queue;       /* GetRSSCPUCore() queue for rss */
	uint8_t  tcp_flags;   /* TCP flags byte (header byte 13); 0 if not TCP */
	uint8_t  ihl_doff;    /* (ihl << 4) | doff; doff 0 if not TCP */
} mosrx_result;

/* Compact 8-byte record (opt-in, mosrx_classify_dev_compact / MOSRX_QUEUE_COMPACT):
 * what an rx loop that keeps no per-frame checksum values reads of a record --
 * the hash and queue (GetRSSHash / GetRSSCPUCore), the reason code and verdict
 * (ProcessPacket's return), the TCP flags byte.  Field for field equal to the
 * same fields of the 16-byte record; half the bytes written per frame, which
 * is a tenth of the HBM traffic of a 64 B frame (BASELINE config #2). */
typedef struct mosrx_result8 {
	uint32_t rss;
	uint8_t  reason;
	uint8_t  queue;
	int8_t   verdict;
	uint8_t  tcp_flags;
} mosrx_result8;

/* pkt_info's TCP fields (mos_api.h:122-152) as FillPacketContextTCPInfo
 * (tcp.c:258-270) fills them, for FindStream and the flow engine after it
 * (tcp.c:448): host order.  12 bytes per frame, an optional side array of the
 * classify calls (_ex); all zero where the record's payload_off is 0. */
typedef struct mosrx_tcpinfo {
	uint32_t seq;         /* ntohl(tcph->seq) */
	uint32_t ack_seq;     /* ntohl(tcph->ack_seq) */
	uint16_t window;      /* ntohs(tcph->window) */
	uint16_t ip_len;      /* pkt_info.ip_len = ntohs(iph->tot_len) (ip_in.c:36, :53) */
} mosrx_tcpinfo;

/* ---- parameters: the reference stack state the verdict depends on --------- */

enum { MOSRX_QMAP_I40E = 1, MOSRX_QMAP_IXGBE = 0 };  /* FetchEndianType() values, config.c:1261-1278 */

#define MOSRX_RSS_KEY_MAX 52   /* the DPDK backend programs a 52-byte key (dpdk_module.c:652-662) */
#define MOSRX_MAX_LOCAL   16   /* netdev entries, MAX_ETH_ENTRY = MAX_DEVICES (config.h:15, io_module.h:87) */

typedef struct mosrx_params {
	uint32_t num_msp;        /* # MOS_SOCK_MONITOR_STREAM sockets (mtcp.h:243); simple_firewall: 1 */
	uint32_t num_esp;        /* # MOS_SOCK_STREAM sockets (mtcp.h:244) */
	int32_t  forward;        /* mos.conf `forward` (config.c:608); setup.sh writes 1 */
	int32_t  num_queues;     /* GetRSSCPUCore num_queues, 1..256 (pcap: 1, pcap_module.c:159) */
	int32_t  queue_mode;     /* MOSRX_QMAP_I40E (non-DPDK default) or MOSRX_QMAP_IXGBE */
	int32_t  skip_tcp_csum;  /* 1: header parse + IP checksum + RSS only (BASELINE config #2) */
	uint32_t rss_key_len;    /* >= 16; only key bytes 0..15 affect a 12-byte input (util.c:47-57) */
	uint8_t  rss_key[MOSRX_RSS_KEY_MAX];
	/* the netdevs' IPv4 addresses (netdev_table->ent[i]->ip_addr, network order as
	 * stored, config.h:54-60): ProcessICMPPacket takes ICMP frames to one of them
	 * (icmp.c:193-200) and ProcessPacket then returns 1 instead of 0 */
	uint32_t num_local;      /* 0..MOSRX_MAX_LOCAL */
	uint32_t local_ip[MOSRX_MAX_LOCAL];
} mosrx_params;

/* simple_firewall's state: num_msp=1, num_esp=0, forward=1, num_queues=1,
 * i40e map, the all-0x05 40-byte key of util.c:36-42. */
void mosrx_params_default(mosrx_params *p);
/* The Microsoft reference Toeplitz key (util/rss.c:75-81), for the MSDN vectors. */
void mosrx_params_set_ms_key(mosrx_params *p);

/* ---- a batch of frames ---------------------------------------------------- */

/* Frame i occupies frames[off[i] .. off[i]+len[i]).  The fast layout puts each
 * frame at a 16-byte boundary + 2 (IP header 16-byte aligned); any offset is
 * accepted.  Offsets are relative to `frames`; frames_bytes bounds every read
 * (the kernel never touches memory outside [frames, frames+frames_bytes)). */
/* Largest batch buffer: its 16-byte-rounded range stays below the offset the
 * kernels use for "no load" (0xFFFFFFF0), so no rounding can wrap. */
#define MOSRX_MAX_FRAMES_BYTES 0xFFFFFFE0ull

typedef struct mosrx_batch {
	const uint8_t  *frames;       /* device pointer (classify_dev) or host pointer (classify_host) */
	uint64_t        frames_bytes; /* <= MOSRX_MAX_FRAMES_BYTES, else -E2BIG */
	const uint32_t *off;          /* n frame offsets */
	const uint16_t *len;          /* n capture lengths (pcap caplen / get_rptr *len, core.c:903-905) */
	uint32_t        n;            /* frames in the batch */
	uint32_t        max_len;      /* max(len[]) if known, else 0 (selects the kernel variant) */
	/* Layout hint (ABI 3).  MOSRX_BATCH_UNIFORM: the producer packed the frames
	 * at a fixed stride, frame i at off0 + i * stride (an rx ring of fixed-size
	 * buffers, a stage of equal-size frames).  The kernel then issues each
	 * frame's header loads from that address together with its descriptor
	 * loads instead of behind them; off[] still decides: a frame whose off[i]
	 * differs is re-read from off[i], so a wrong hint costs time, never a
	 * result.  Used when off0 and stride fit 16 bits; 0 = no hint. */
	uint32_t        layout;       /* MOSRX_BATCH_* */
	uint32_t        off0;
	uint32_t        stride;
	uint32_t        reserved;     /* 0 */
} mosrx_batch;
enum { MOSRX_BATCH_UNIFORM = 1 };

typedef struct mosrx_ctx mosrx_ctx;

/* Open a context on HIP device `device`.  Fails with -ENODEV when no GPU or
 * the HIP kernels are unavailable: there is no CPU fallback. */
int  mosrx_open(int device, const mosrx_params *p, mosrx_ctx **out);
/* Visible HIP devices (0 without a GPU or runtime). */
int  mosrx_device_count(void);
int  mosrx_set_params(mosrx_ctx *c, const mosrx_params *p);
/* Tuning knob (0..127; results never depend on it): bit 1 = non-temporal tail
 * stream (bit 0, non-temporal header windows, measured slower and folded onto
 * bit 1's setting); bits 2-6 = force a kernel shape (value - 1; 0 = automatic).
 * Default from measurements; env MOSRX_KVARIANT overrides at open. */
int  mosrx_set_variant(mosrx_ctx *c, int variant);
void mosrx_close(mosrx_ctx *c);

/* Device-resident classification: `b` points at device memory, results go to
 * device memory `d_out[n]`.  Enqueued on `stream` (a hipStream_t, NULL = the
 * context's own stream); returns after enqueue.  Graph-capturable. */
int  mosrx_classify_dev(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *d_out, void *stream);

/* Same, plus the flow-table hash of every frame into device memory
 * `d_fhash[n]`: SuperFastHash of FindStream's reversed tuple (tcp.c:185-190,
 * fhash.c:25-92) before the NUM_BINS mask, i.e. HashFlow() == d_fhash[i] &
 * 0x1FFFF.  0 where payload_off == 0 (no TCP header).  Replaces the per-packet
 * HashFlow call of HTSearch (fhash.c:184-203) with a precomputed bucket. */
int  mosrx_classify_dev_fh(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *d_out, uint32_t *d_fhash,
                           void *stream);

/* Same, with every optional per-frame side array: d_fhash[n] (NULL: none, as
 * above) and d_tcpinfo[n] (NULL: none), the pkt_info TCP fields, computed in the
 * same pass from the header bytes the kernel already holds. */
int  mosrx_classify_dev_ex(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *d_out, uint32_t *d_fhash,
                           mosrx_tcpinfo *d_tcpinfo, void *stream);

/* Same with 8-byte records into device memory d_out8[n] (8-byte aligned). */
int  mosrx_classify_dev_compact(mosrx_ctx *c, const mosrx_batch *b, mosrx_result8 *d_out8, void *stream);

/* Device-resident classification of `nb` batches in one launch sequence. */
int  mosrx_classify_dev_many(mosrx_ctx *c, const mosrx_batch *b, uint32_t nb,
                             mosrx_result *const *d_out, void *stream);

/* Batch queue: a device-resident descriptor table of `nb` resident batches
 * that ONE kernel launch classifies (a workgroup finds its batch by binary
 * search).  Amortises launch latency for small batches (64 B frames, 32K per
 * batch); every batch keeps its own frames, descriptors and result buffer. */
typedef struct mosrx_queue mosrx_queue;
int  mosrx_queue_create(mosrx_ctx *c, const mosrx_batch *b, uint32_t nb,
                        mosrx_result *const *d_out, mosrx_queue **q);
int  mosrx_queue_run(mosrx_ctx *c, const mosrx_queue *q, void *stream);
void mosrx_queue_destroy(mosrx_ctx *c, mosrx_queue *q);
/* The batch queue with its options: d_out[i] points at 16-byte records, or at
 * 8-byte ones (mosrx_result8) with MOSRX_QUEUE_COMPACT; d_fhash[i] (NULL: none)
 * the flow-table hashes; d_match[i] (NULL: none) the match masks of the BPF set
 * installed when the queue runs -- one launch of the fused classify + BPF
 * queue kernel when the set has its compiled form, else the classify launch
 * followed by the set's kernel per batch (same results).  Compact records go
 * with both side arrays (the fused kernels have 8-byte forms). */
enum { MOSRX_QUEUE_COMPACT = 1 };
int  mosrx_queue_create_ex(mosrx_ctx *c, const mosrx_batch *b, uint32_t nb, void *const *d_out,
                           uint32_t *const *d_fhash, uint32_t *const *d_match, int flags, mosrx_queue **q);
/* `iters` back-to-back launches cycling over `nq` queues; HIP events on the
 * kernel stream (total, and per launch for the average kernel duration). */
int  mosrx_time_queue(mosrx_ctx *c, mosrx_queue *const *q, uint32_t nq, uint32_t iters,
                      float *total_ms, float *avg_kernel_ms);

/* ---- queue steering: the per-core sort a NIC's RSS does ------------------- */
/* A stable partition of a batch's frame indices by the records' `queue` byte
 * (GetRSSCPUCore, util.c:114-131), computed on the GPU from the records a
 * classify call wrote:
 *   idx[n]                       batch-local frame indices grouped by queue,
 *                                ascending within a queue (arrival order kept)
 *   qstart[MOSRX_STEER_QSLOTS]   queue q's frames are idx[qstart[q] .. qstart[q+1]),
 *                                qstart[256] == n
 * The slot count does not depend on num_queues (the key is a byte, so no
 * record value indexes outside qstart): with num_queues = 8, entries 8..256
 * all equal n.  Each mTCP thread owns the flows whose hash maps to its core
 * (and api.c:1056 picks source ports to match); this is that map applied to a
 * batch from a single ingress.  Three kernel launches (histogram, scan,
 * scatter) behind the classify launch on the same stream. */
#define MOSRX_STEER_QSLOTS 257
/* Scratch a steer of n frames needs (no GPU needed; never 0, non-decreasing
 * in n), and the frames one workgroup takes. */
size_t   mosrx_steer_scratch_bytes(uint32_t n);
uint32_t mosrx_steer_tile(void);
/* Steer one device-resident batch: d_rec are its n records of rec_bytes (16:
 * mosrx_result, 8: mosrx_result8) as a classify call on the same stream left
 * them; d_idx[n], d_qstart[MOSRX_STEER_QSLOTS] and d_scratch (4-byte aligned,
 * at least mosrx_steer_scratch_bytes(n)) are the caller's, so the call
 * allocates nothing and is graph-capturable.  -EINVAL: rec_bytes not 8 or 16,
 * a NULL or misaligned pointer, scratch too small.  n == 0 returns 0 and
 * launches nothing. */
int  mosrx_steer_dev(mosrx_ctx *c, const void *d_rec, uint32_t n, int rec_bytes, uint32_t *d_idx,
                     uint32_t *d_qstart, void *d_scratch, size_t scratch_bytes, void *stream);
/* Attach per-batch steer outputs to a batch queue (d_idx[i]: n_i entries,
 * NULL allowed for an empty batch; d_qstart[i]: MOSRX_STEER_QSLOTS): every
 * mosrx_queue_run then enqueues the three steer launches behind the classify
 * launch on the same stream.  The queue's scratch is allocated at the first
 * attach.  Both NULL detaches: the queue runs exactly as before.  Not while a
 * run of the queue is in flight. */
int  mosrx_queue_set_steer(mosrx_ctx *c, mosrx_queue *q, uint32_t *const *d_idx, uint32_t *const *d_qstart);
/* Arm the next group submit on `slot` (any mosrx_classify_host_group_submit*
 * variant), once: the steer launches follow the group's classify launch on
 * the slot's stream, batch i's outputs land in h_idx[i] (n_i entries) and
 * h_qstart[i] (MOSRX_STEER_QSLOTS) by the rule of the other output arrays --
 * written in place for a direct group whose outputs (these included) are all
 * pinned, else copied back with the records.  The two pointer arrays must
 * stay valid until that submit returns.  The slot's steer buffers are part of
 * mosrx_classify_host_reserve, so arming never makes a slot grow in traffic.
 * Both NULL disarms.  -EBUSY while the slot runs. */
int  mosrx_slot_steer(mosrx_ctx *c, int slot, uint32_t *const *h_idx, uint32_t *const *h_qstart);

/* ---- queue-major gather: each queue's share as contiguous runs -------------- */
/* The steer forms with extra outputs in the order of idx, written by the
 * scatter launch (its gather form; histogram and scan are the same launches):
 *   qrec[n * rec_bytes]   qrec[j] = rec[idx[j]], whole records
 *   qoff[n], qlen[n]      off[idx[j]], len[idx[j]] of the batch's descriptors;
 *                         both given or both NULL (NULL: records only)
 * Queue q's share of the batch is then three contiguous runs from qstart[q]:
 * over the batch's frame buffer, a batch in the library's own descriptor form,
 * the ring a NIC would have filled for that core.  rec and qrec must be
 * aligned to rec_bytes, qoff (and off) to 4, qlen (and len) to 2: -EINVAL
 * otherwise.  Per frame the pass reads 6 more bytes and writes rec_bytes + 6
 * more than the plain scatter. */
/* mosrx_steer_dev with the gather outputs; d_off / d_len are the batch's
 * descriptors (may be NULL with d_qoff / d_qlen NULL).  Same scratch
 * (mosrx_steer_scratch_bytes), allocates nothing, graph-capturable; n == 0
 * returns 0 and launches nothing. */
int  mosrx_steer_gather_dev(mosrx_ctx *c, const void *d_rec, const uint32_t *d_off, const uint16_t *d_len,
                            uint32_t n, int rec_bytes, uint32_t *d_idx, uint32_t *d_qstart, void *d_qrec,
                            uint32_t *d_qoff, uint16_t *d_qlen, void *d_scratch, size_t scratch_bytes,
                            void *stream);
/* mosrx_queue_set_steer with per-batch gather outputs (d_qrec[i]: n_i records
 * of the queue's record size; d_qoff / d_qlen: both arrays or both NULL); the
 * descriptors gathered are the queue's own batches'.  All five NULL detaches,
 * as mosrx_queue_set_steer(c, q, NULL, NULL) does. */
int  mosrx_queue_set_steer_gather(mosrx_ctx *c, mosrx_queue *q, uint32_t *const *d_idx, uint32_t *const *d_qstart,
                                  void *const *d_qrec, uint32_t *const *d_qoff, uint16_t *const *d_qlen);
/* mosrx_slot_steer with gather outputs, under its rules: one-shot, written in
 * place for a direct group whose outputs (these included) are all pinned, else
 * copied back with the records; the slot's gather buffers are part of
 * mosrx_classify_host_reserve.  All five NULL disarms. */
int  mosrx_slot_steer_gather(mosrx_ctx *c, int slot, uint32_t *const *h_idx, uint32_t *const *h_qstart,
                             void *const *h_qrec, uint32_t *const *h_qoff, uint16_t *const *h_qlen);

/* ---- the gather's side form: a batch's other per-frame outputs in queue order -- */
/* The gather forms with up to three more arrays stored in the order of idx by
 * the same launch (its side form; no further launch, histogram and scan as
 * they are):
 *   qfhash[j]   = fhash[idx[j]]     the flow-table hashes (u32)
 *   qmatch[j]   = match[idx[j]]     the BPF match masks (u32)
 *   qtcpinfo[j] = tcpinfo[idx[j]]   mosrx_tcpinfo, whole
 * so queue q's hashes, masks and pkt_info are contiguous runs from qstart[q],
 * beside its records.  Each array on its own: a NULL destination is not
 * gathered (nothing read, nothing written); with none given the launch is the
 * plain gather form.  All pointers 4-byte aligned.  Per frame the pass reads
 * and writes 4 more bytes for a u32 array, 12 for tcpinfo. */
/* mosrx_steer_gather_dev plus the three source / destination pairs (both
 * pointers of a pair or neither: -EINVAL otherwise).  Same scratch, allocates
 * nothing, graph-capturable; n == 0 returns 0 and launches nothing. */
int  mosrx_steer_gather_side_dev(mosrx_ctx *c, const void *d_rec, const uint32_t *d_off, const uint16_t *d_len,
                                 uint32_t n, int rec_bytes, uint32_t *d_idx, uint32_t *d_qstart, void *d_qrec,
                                 uint32_t *d_qoff, uint16_t *d_qlen, const uint32_t *d_fhash, uint32_t *d_qfhash,
                                 const uint32_t *d_match, uint32_t *d_qmatch, const mosrx_tcpinfo *d_tcpinfo,
                                 mosrx_tcpinfo *d_qtcpinfo, void *d_scratch, size_t scratch_bytes, void *stream);
/* mosrx_queue_set_steer_gather plus per-batch d_qfhash / d_qmatch (either may
 * be NULL); the sources are the queue's own d_fhash / d_match of
 * mosrx_queue_create_ex, and a destination for an array the queue does not
 * produce is -EINVAL.  All seven NULL detaches. */
int  mosrx_queue_set_steer_gather_side(mosrx_ctx *c, mosrx_queue *q, uint32_t *const *d_idx,
                                       uint32_t *const *d_qstart, void *const *d_qrec, uint32_t *const *d_qoff,
                                       uint16_t *const *d_qlen, uint32_t *const *d_qfhash,
                                       uint32_t *const *d_qmatch);
/* mosrx_slot_steer_gather plus h_qfhash / h_qmatch / h_qtcpinfo (any may be
 * NULL), under its rules.  The armed submit gathers each side array it makes
 * itself for which a destination was given -- flow hashes with h_fhash, masks
 * on the _bpf / _bpf_c8 submits, pkt_info with h_tcpinfo -- and leaves the
 * other destinations untouched.  The slot's buffers for them are part of
 * mosrx_classify_host_reserve.  All eight NULL disarms. */
int  mosrx_slot_steer_gather_side(mosrx_ctx *c, int slot, uint32_t *const *h_idx, uint32_t *const *h_qstart,
                                  void *const *h_qrec, uint32_t *const *h_qoff, uint16_t *const *h_qlen,
                                  uint32_t *const *h_qfhash, uint32_t *const *h_qmatch,
                                  mosrx_tcpinfo *const *h_qtcpinfo);
#define MOSRX_SIDE_FHASH   1   /* the side arrays, as bits (MOSRX_OP_STEER_GATHER_SIDE's arg) */
#define MOSRX_SIDE_MATCH   2
#define MOSRX_SIDE_TCPINFO 4

/* ---- the one-launch steer form: small batches, direct groups ----------------- */
/* Histogram, scan and scatter (or its gather / side form) in one kernel, one
 * workgroup per batch, for batches whose steering is bound by launch latency
 * rather than by the walk: the same outputs as the three launches, bit for
 * bit.  Per context and off by default: with a limit of max_frames > 0 every
 * steer entry point (mosrx_steer_dev and its gather / side forms, a steered
 * mosrx_queue_run, an armed group submit, the MOSRX_OP_STEER* timing ops)
 * issues the one launch when every batch of that launch has n <= max_frames,
 * and the three launches otherwise (one larger batch sends the whole launch
 * there).  0: the three launches, always.  MOSRX_STEER_ONE_MAX bounds one
 * workgroup's walk (32 tiles); a limit above it is -EINVAL and changes
 * nothing.  The limit worth setting is far smaller: DESIGN.md §4.12.  The
 * device calls still take (and in this form leave untouched) their scratch. */
#define MOSRX_STEER_ONE_MAX 65536u
int      mosrx_set_steer_one(mosrx_ctx *c, uint32_t max_frames);
uint32_t mosrx_get_steer_one(const mosrx_ctx *c);
/* Steer launches of this context that took the one-launch form so far. */
uint64_t mosrx_steer_one_count(const mosrx_ctx *c);

/* ---- forwarding: the frames a forward = 1 stack passes on -------------------- */
/* What ProcessPacket does with a frame it does not keep: ForwardIPPacket
 * (ip_out.c:39-110: GetOutputInterface's longest-prefix walk, ip_out.c:11-37;
 * GetDestinationHWaddr's, arp.c:88-119; EthernetOutput's 14-byte header,
 * eth_out.c:62-102; a memcpy of the IP packet) or ForwardEthernetFrame
 * (eth_out.c:104-134), over a classified batch: a plan record per frame, then
 * the TX frames mOS would have put on the wire, byte for byte, in arrival
 * order.  Stateless per launch: the tables are the fields mOS holds after it
 * parsed mos.conf, taken verbatim (addresses in network order as struct
 * route_entry / struct _arp_entry keep them; no mask is recomputed here). */
#define MOSRX_FWD_MAX_ROUTES  128    /* MAX_ROUTE_ENTRY */
#define MOSRX_FWD_MAX_ARP     1024   /* MAX_ARPENTRY */
#define MOSRX_FWD_MAX_NETDEVS 16
typedef struct mosrx_fwd_route {
	uint32_t mask, masked_ip;
	int32_t  prefix, nif;            /* nif: an index into the netdevs */
} mosrx_fwd_route;
typedef struct mosrx_fwd_arp {
	uint32_t ip, mask, masked_ip;
	int32_t  prefix;
	uint8_t  haddr[6];
	uint8_t  pad[2];
} mosrx_fwd_arp;
typedef struct mosrx_fwd_tables {
	uint32_t num_routes;             /* <= MOSRX_FWD_MAX_ROUTES */
	uint32_t num_arp;                /* <= MOSRX_FWD_MAX_ARP */
	uint32_t num_netdevs;            /* <= MOSRX_FWD_MAX_NETDEVS */
	int32_t  has_nic_fwd;            /* g_config.mos->nic_forward_table != NULL */
	int8_t   nic_fwd[MOSRX_FWD_MAX_NETDEVS];   /* nic_fwd_table[in_ifidx]: an output netdev or -1 */
	uint8_t  netdev_haddr[MOSRX_FWD_MAX_NETDEVS][6];
	mosrx_fwd_route routes[MOSRX_FWD_MAX_ROUTES];
	mosrx_fwd_arp   arp[MOSRX_FWD_MAX_ARP];
} mosrx_fwd_tables;

/* The plan of one frame, 8 bytes. */
enum {
	MOSRX_FWD_NONE     = 0,  /* not forwarded (mosrx_mos_forwards' rule; TRUNCATED never is) */
	MOSRX_FWD_IP       = 1,  /* ForwardIPPacket sends 14 + ntohs(tot_len) bytes */
	MOSRX_FWD_ETH      = 2,  /* ForwardEthernetFrame sends the frame as captured */
	MOSRX_FWD_NO_ROUTE = 3,  /* GetOutputInterface found no route */
	MOSRX_FWD_NO_ARP   = 4,  /* GetDestinationHWaddr found no entry (forward = 1: no ARP request, ip_out.c:69) */
	MOSRX_FWD_NO_NIC   = 5   /* no nic_forward_table, or its entry is -1 (non-IPv4 frames) */
};
typedef struct mosrx_fwd {
	uint16_t tx_len;      /* bytes sent; 0 unless kind is IP or ETH */
	int8_t   out_ifidx;   /* the output netdev (IP, ETH, NO_ARP), else -1 */
	uint8_t  kind;        /* MOSRX_FWD_* */
	uint16_t arp_idx;     /* the ARP entry GetDestinationHWaddr picked; 0xFFFF: none (the frame keeps its h_dest) */
	uint16_t reserved;    /* 0 */
} mosrx_fwd;

/* Validate the tables and upload one packed device copy for the context:
 * -EINVAL when a count is over its limit, a route's nif or a nic_fwd entry
 * (other than -1) is outside the netdevs.  NULL clears them.  In effect for
 * launches submitted after it returns; launches already submitted keep the
 * copy they were given (a device copy is rewritten only after they drained). */
int  mosrx_fwd_set(mosrx_ctx *c, const mosrx_fwd_tables *t);
/* 1 when an end-host socket listens (mtcp->listener): TCP frames of flows
 * without a stream are then answered, not forwarded (tcp.c:453-510).  0 at open. */
int  mosrx_fwd_set_listener(mosrx_ctx *c, int listener);
/* Plan a device-resident batch from its n records of rec_bytes (16 or 8) as a
 * classify call on the same stream left them, under the context's forward /
 * num_msp and the listener flag; in_ifidx is the batch's input netdev.  One
 * launch into d_plan[n] (8-byte aligned).  Allocates nothing, graph-capturable.
 * -EINVAL: NULL or misaligned pointer, rec_bytes, in_ifidx outside
 * 0 .. MOSRX_FWD_MAX_NETDEVS - 1; -ENOENT: no tables set.  n == 0 returns 0
 * and launches nothing. */
int  mosrx_fwd_plan_dev(mosrx_ctx *c, const mosrx_batch *b, const void *d_rec, int rec_bytes, int in_ifidx,
                        mosrx_fwd *d_plan, void *stream);
/* Build the TX frames of a planned batch, in arrival order: sent frame j
 * (kind IP or ETH) at tx_off[j] = 16 k + 2 (the library's staging convention:
 * the IP header on a 16-byte boundary), k the exclusive scan of
 * ceil((2 + tx_len) / 16) over the sent frames.  An IP frame is h_dest (the
 * ARP entry's, or its own on the nic_forward_table path), h_source = the output
 * netdev's haddr, its ethertype, then tx_len - 14 bytes from frame byte 14;
 * an ETH frame is copied unchanged.
 *   d_tx_frames[tx_cap]  16-byte aligned; only frame bytes are written
 *   d_tx_off / d_tx_len / d_tx_nif / d_tx_src [m]   src: the frame's index in the batch
 *   d_tx_count[2]        {m, frames dropped for lack of room}
 * A frame whose padded end passes tx_cap is not written and counted dropped,
 * and so is every later one.  Entries past m and bytes past the last frame
 * are left untouched; the four arrays need room for n entries.  Three launches
 * (totals, scan, copy) on one stream; allocates nothing, graph-capturable.
 * -EINVAL: NULL or misaligned pointer, scratch under mosrx_fwd_scratch_bytes(n);
 * -ENOENT: no tables set. */
int  mosrx_fwd_build_dev(mosrx_ctx *c, const mosrx_batch *b, const mosrx_fwd *d_plan, uint8_t *d_tx_frames,
                         uint64_t tx_cap, uint32_t *d_tx_off, uint16_t *d_tx_len, int8_t *d_tx_nif,
                         uint32_t *d_tx_src, uint32_t *d_tx_count, void *d_scratch, size_t scratch_bytes,
                         void *stream);
/* Scratch a build of n frames needs (no GPU needed; never 0, non-decreasing in
 * n; 16-byte aligned at the call), and the frames one workgroup takes. */
size_t   mosrx_fwd_scratch_bytes(uint32_t n);
uint32_t mosrx_fwd_tile(void);

/* The ring form of the build: the same frames, byte for byte, each in the TX
 * ring of its output netdev, as a NIC's TX queues would hold them (mOS sends
 * per netdev: get_wptr(ctx, nif, len) / send_pkts(ctx, nif)).  A frame is sent
 * when its kind is IP or ETH, tx_len >= 14 and out_ifidx is in 0 .. nrings - 1.
 *   ring q      d_tx_frames[q * ring_cap .. (q + 1) * ring_cap)
 *   its r-th sent frame, in arrival order, at q * ring_cap + 16 k + 2, k the
 *               exclusive scan of ceil((2 + tx_len) / 16) over netdev q's sent
 *               frames alone
 *   its entry   j = rings[q].start + r: tx_off[j] (from d_tx_frames), tx_len[j],
 *               tx_src[j] (the frame's index in the batch); the ring says the netdev
 * A frame whose padded end passes ring_cap is not written and counted in
 * rings[q].dropped, and so is every later frame of that netdev; other netdevs
 * are not affected.  Ring q's written frames are entries start .. start + count;
 * entries start + count .. start + count + dropped are left untouched, as are
 * padding, ring bytes past 16 * units, entries past the last ring and
 * d_rings[nrings ..].  d_rings[0 .. nrings) is written whole by every call
 * (n == 0 included); the three entry arrays need room for n entries.  Three
 * launches on one stream; allocates nothing, graph-capturable.
 * -EINVAL: NULL or misaligned pointer (d_tx_frames, d_rings, d_scratch to 16
 * bytes, d_tx_off / d_tx_src to 4, d_tx_len to 2), nrings outside
 * 1 .. MOSRX_FWD_MAX_NETDEVS or below the installed tables' num_netdevs,
 * ring_cap not a multiple of 16 or nrings * ring_cap > 2^32 (tx_off is 32
 * bits), scratch under mosrx_fwd_rings_scratch_bytes(n, nrings); -ENOENT: no
 * tables set. */
typedef struct mosrx_fwd_ring {   /* 16 bytes, one per output netdev */
	uint32_t start;     /* first entry of this netdev in tx_off / tx_len / tx_src */
	uint32_t count;     /* frames written to the ring */
	uint32_t dropped;   /* sent frames of this netdev that did not fit */
	uint32_t units;     /* 16-byte units the written frames take: the ring is filled to 16 * units */
} mosrx_fwd_ring;
int    mosrx_fwd_build_rings_dev(mosrx_ctx *c, const mosrx_batch *b, const mosrx_fwd *d_plan,
                                 uint8_t *d_tx_frames, uint64_t ring_cap, uint32_t nrings,
                                 uint32_t *d_tx_off, uint16_t *d_tx_len, uint32_t *d_tx_src,
                                 mosrx_fwd_ring *d_rings, void *d_scratch, size_t scratch_bytes, void *stream);
/* Scratch a ring build needs (no GPU needed; never 0, non-decreasing in both). */
size_t mosrx_fwd_rings_scratch_bytes(uint32_t n, uint32_t nrings);

/* Forwarding attached to a batch queue, the way steering is: every
 * mosrx_queue_run then enqueues, behind the classify launch (and the steer
 * launches) on the same stream, one plan launch over every batch of the queue
 * and, with TX outputs given, the ring build's three launches over every
 * batch: four launches per run whatever nb is.  Batch i's outputs are byte
 * for byte what mosrx_fwd_plan_dev + mosrx_fwd_build_rings_dev write for that
 * batch alone under the same tables, ring_cap and nrings.  The records read
 * are the queue's own (8-byte with MOSRX_QUEUE_COMPACT, else 16-byte).
 *   in_ifidx     nb input netdevs, 0 .. MOSRX_FWD_MAX_NETDEVS - 1; NULL: all 0
 *   d_plan       nb plan arrays, d_plan[i]: n_i entries, 8-byte aligned (NULL
 *                allowed for an empty batch only)
 *   ring_cap, nrings   as mosrx_fwd_build_rings_dev, the same for every batch
 *   d_tx_frames  nb ring blocks of nrings * ring_cap bytes, 16-byte aligned
 *   d_tx_off, d_tx_len, d_tx_src   n_i entries each
 *   d_rings      d_rings[i][nrings], 16-byte aligned; required for empty
 *                batches too, and written {0, 0, 0, 0} for them
 * The five TX pointer arrays are all NULL (plan only: ring_cap and nrings are
 * not looked at) or all non-NULL.  f == NULL detaches: the queue runs exactly
 * as before.  Not while a run of the queue is in flight.  The queue's device
 * table and scratch (a row of MOSRX_FWD_ROW bytes per tile and ring) are
 * allocated at the first attach that needs them and freed by
 * mosrx_queue_destroy.  -EINVAL (the queue keeps the attachment it had): a
 * NULL or misaligned pointer of a non-empty batch, an in_ifidx out of range,
 * half a set of TX arrays, nrings outside 1 .. MOSRX_FWD_MAX_NETDEVS, ring_cap
 * not a multiple of 16 or nrings * ring_cap > 2^32.
 * The tables, forward, num_msp and the listener flag are those in effect at
 * each run, as for mosrx_fwd_plan_dev.  A run of a queue with forwarding
 * attached checks before it launches anything: -ENOENT with no tables
 * installed, -EINVAL with TX outputs attached and nrings below the installed
 * tables' num_netdevs; nothing is enqueued then, not even the classify launch. */
typedef struct mosrx_queue_fwd {
	const uint8_t *in_ifidx;
	mosrx_fwd *const *d_plan;
	uint64_t  ring_cap;
	uint32_t  nrings;
	uint8_t        *const *d_tx_frames;
	uint32_t       *const *d_tx_off;
	uint16_t       *const *d_tx_len;
	uint32_t       *const *d_tx_src;
	mosrx_fwd_ring *const *d_rings;
} mosrx_queue_fwd;
int mosrx_queue_set_fwd(mosrx_ctx *c, mosrx_queue *q, const mosrx_queue_fwd *f);

/* The descriptor form of the ring build, for a host that still holds the
 * received frames (the drop-in backend's staging, a pinned source ring): what
 * it lacks per sent frame, 18 bytes, in place of the frame.  The sent rule and
 * the entry order are the ring form's: ring q's r-th sent frame, in arrival
 * order, has entry e = rings[q].start + r, and
 *   d_tx_src[e]   u32   the frame's index in the batch
 *   d_tx_len[e]   u16   its TX length
 *   d_tx_mac[e]   12 bytes (three dwords, 4-byte aligned): h_dest then h_source,
 *                 bytes 0 .. 11 of the frame mosrx_fwd_build_rings_dev writes --
 *                 kind IP: a_haddr[arp_idx] (the frame's own h_dest when arp_idx
 *                 is 0xFFFF, the nic_forward_table path) then
 *                 netdev_haddr[out_ifidx]; kind ETH: the frame's own bytes
 *   d_rings[q]    {start, count, dropped = 0, units}: start the sent frames of
 *                 the netdevs below q, units the sum of ceil((2 + tx_len) / 16)
 *                 over the ring's frames -- what a byte ring large enough to drop
 *                 nothing reports, so a host can size one
 * There is no capacity and nothing is dropped.  d_rings[0 .. nrings) is written
 * whole by every call (n == 0 included: zeroes); entries at and past the total
 * sent count and d_rings[nrings ..] are left untouched; the three entry arrays
 * need room for n entries.  Three launches on one stream (the ring form's
 * totals and scan, then a store launch); allocates nothing, graph-capturable.
 * -EINVAL: NULL or misaligned pointer (d_rings, d_scratch to 16 bytes, d_tx_src /
 * d_tx_mac to 4, d_tx_len to 2), nrings outside 1 .. MOSRX_FWD_MAX_NETDEVS or
 * below the installed tables' num_netdevs, scratch under
 * mosrx_fwd_desc_scratch_bytes(n, nrings); -ENOENT: no tables set.  A refused
 * call launches nothing. */
int    mosrx_fwd_desc_rings_dev(mosrx_ctx *c, const mosrx_batch *b, const mosrx_fwd *d_plan, uint32_t nrings,
                                uint32_t *d_tx_src, uint16_t *d_tx_len, uint32_t *d_tx_mac, mosrx_fwd_ring *d_rings,
                                void *d_scratch, size_t scratch_bytes, void *stream);
size_t mosrx_fwd_desc_scratch_bytes(uint32_t n, uint32_t nrings);

/* The descriptor form attached to a batch queue: every mosrx_queue_run then
 * enqueues the plan launch and the descriptor form's three over every batch,
 * four launches whatever nb is; batch i's outputs are byte for byte those of
 * mosrx_fwd_plan_dev + mosrx_fwd_desc_rings_dev on that batch alone.  Fields
 * and rules as mosrx_queue_fwd's: d_plan[i] / d_tx_src[i] / d_tx_len[i] /
 * d_tx_mac[i] may be NULL for an empty batch only, d_rings[i] is required for
 * every batch; everything is validated before anything changes; f == NULL
 * detaches.  A queue carries either this attachment or mosrx_queue_set_fwd's:
 * attaching one while the other is attached is -EINVAL.  A run checks before it
 * launches anything: -ENOENT with no tables installed, -EINVAL with nrings below
 * the installed tables' num_netdevs; nothing is enqueued then. */
typedef struct mosrx_queue_fwd_desc {
	const uint8_t *in_ifidx;
	mosrx_fwd *const *d_plan;
	uint32_t  nrings;
	uint32_t       *const *d_tx_src;
	uint16_t       *const *d_tx_len;
	uint32_t       *const *d_tx_mac;
	mosrx_fwd_ring *const *d_rings;
} mosrx_queue_fwd_desc;
int mosrx_queue_set_fwd_desc(mosrx_ctx *c, mosrx_queue *q, const mosrx_queue_fwd_desc *f);

/* The same attached to the next group submit on `slot`, once, the way
 * mosrx_slot_steer* arm it (and together with such an arm, or alone): the plan
 * and descriptor launches follow the group's classify launch, and the steer
 * launches if armed, on the slot's stream, with any
 * mosrx_classify_host_group_submit* variant (16- or 8-byte records).  Batch i's
 * outputs land in h_tx_src[i] / h_tx_len[i] / h_tx_mac[i] (n_i entries each; 4-,
 * 2-, 4-byte aligned; may be NULL for an empty batch), h_rings[i][nrings]
 * (required for every batch) and, when h_plan is given, h_plan[i] (8-byte
 * aligned).  Placement follows the other outputs' rule: written in place for a
 * direct group whose outputs, these included (h_rings 16-byte aligned), are all
 * pinned -- then byte for byte mosrx_fwd_desc_rings_dev's -- otherwise copied
 * back with the records: all n_i entries of each array are then overwritten,
 * and those at and past the sent count hold nothing of meaning.  A group of
 * empty batches gets its zeroed rings.  The pointer arrays must stay valid
 * until the submit.  in_ifidx: nb input netdevs, NULL: all 0.  The slot's device
 * buffers are part of mosrx_classify_host_reserve.  o == NULL disarms.
 * -EBUSY while the slot runs; -ENOENT without tables and -EINVAL for nrings
 * outside 1 .. MOSRX_FWD_MAX_NETDEVS or below num_netdevs or a NULL array, here
 * and again at the submit (the tables in effect then), before anything is
 * submitted. */
typedef struct mosrx_slot_fwd_out {
	const uint8_t *in_ifidx;
	uint32_t  nrings;
	mosrx_fwd      *const *h_plan;
	uint32_t       *const *h_tx_src;
	uint16_t       *const *h_tx_len;
	uint32_t       *const *h_tx_mac;
	mosrx_fwd_ring *const *h_rings;
} mosrx_slot_fwd_out;
int mosrx_slot_fwd(mosrx_ctx *c, int slot, const mosrx_slot_fwd_out *o);

/* ---- the one-launch forwarding form: small batches, direct groups ------------- */
/* The plan and the descriptor rings in one kernel, one workgroup per batch, for
 * batches whose forwarding is bound by launch latency rather than by the walk:
 * the same outputs as the four launches, byte for byte.  Per context and off by
 * default: with a limit of max_frames > 0 every place that issues the plan and
 * the descriptor form together (a mosrx_queue_run with mosrx_queue_set_fwd_desc
 * attached, a group submit armed by mosrx_slot_fwd, MOSRX_OP_FWD_DESC) issues
 * the one launch when every batch of that launch has n <= max_frames, and the
 * four launches otherwise (one larger batch sends the whole launch there);
 * mosrx_fwd_desc_rings_dev takes its plan as given and issues one launch in
 * place of its three, leaving its scratch untouched.  0: the existing
 * launches, always.  MOSRX_FWD_ONE_MAX bounds one workgroup's walk (32 tiles
 * of 256 frames); a limit above it is -EINVAL and changes nothing.  The limit
 * worth setting: DESIGN.md §4.13.  Refusals are those of the entry points and
 * come before any launch.  The byte-ring forms, mosrx_fwd_plan_dev and a
 * plan-only queue attachment are not affected. */
#define MOSRX_FWD_ONE_MAX 8192u
int      mosrx_set_fwd_one(mosrx_ctx *c, uint32_t max_frames);
uint32_t mosrx_get_fwd_one(const mosrx_ctx *c);
/* Forwarding launches of this context that took the one-launch form so far (n == 0 launches included). */
uint64_t mosrx_fwd_one_count(const mosrx_ctx *c);

/* ---- firewall rules on SYN frames, ahead of forwarding ------------------------- */
/* What samples/simple_firewall does to the frames a forward = 1 stack passes
 * on: on a TCP frame with SYN and no ACK (CatchInitSYN, simple_firewall.c:362-372)
 * it walks its rules, first match wins (FWRLookup, :307-330, over MatchAddr /
 * MatchPort, :291-305), counts the hit in the rule (fr_count) and, for a DROP
 * rule, withholds that frame from forwarding (ApplyActionPerFlow, :332-360:
 * mtcp_setlastpkt(MOS_DROP)).  Here as one launch over a classified batch,
 * between the plan launch and the build launches: stateless per frame.
 *
 * A frame is looked up when its record's reason is TCP_OK or TCP_LEN_OK, the
 * context has num_msp != 0 and the listener flag off (the TCP arm of
 * mosrx_mos_forwards), its tcp_flags have SYN and not ACK, and its IPv4 packet
 * lies inside its capture (the plan's condition).  `forward` is no condition:
 * the sample looks up and counts either way.  The key is read from the frame
 * as the sample reads it: saddr / daddr at bytes 26..33, the ports at
 * 14 + 4 * ihl (ihl from byte 14), each the raw value of a little-endian host;
 * a key byte at or past the batch buffer's end (rounded up to 16) reads zero.
 *
 * The boundary: mOS raises the sample's event from inside its stream engine,
 * behind tcp.c:445.  Where that engine would not raise MOS_ON_PKT_IN for an
 * accepted SYN (a retransmitted SYN of a flow it no longer monitors, say), the
 * sample looks nothing up and this launch does.  The ACCEPT branch
 * (MOS_STOP_MON) does nothing to forwarding and is not modelled. */
#define MOSRX_ACL_MAX_RULES 1024   /* MAX_RULES */
enum { MOSRX_ACL_ACCEPT = 1, MOSRX_ACL_DROP = 2 };   /* FRA_ACCEPT, FRA_DROP */
/* One rule: the fields struct FirewallRule holds after ParseConfigFile, network
 * order as stored.  src_ip / dst_ip are already masked (ExtractIPAddress,
 * :204); src_mask / dst_mask are the values IP_NETMASK ands with,
 * 0xFFFFFFFF >> (32 - bits) on the stored address -- for a prefix that is no
 * multiple of 8 that keeps the low bits of the last partial octet, which is the
 * sample's behaviour; no mask is recomputed here.  An address or port of 0 is
 * the wildcard. */
typedef struct mosrx_acl_rule {
	uint32_t src_ip, src_mask, dst_ip, dst_mask;
	uint16_t sport, dport;
	uint8_t  action;      /* MOSRX_ACL_ACCEPT or MOSRX_ACL_DROP */
	uint8_t  pad[3];
} mosrx_acl_rule;
/* The kind the launch gives a dropped SYN's plan record: {tx_len 0, out_ifidx -1,
 * MOSRX_FWD_DROP, arp_idx 0xFFFF, reserved 0}.  Every build sends kinds IP and
 * ETH only, so the frame falls out of all of them. */
#define MOSRX_FWD_DROP 6
/* d_hit values that are no rule index */
#define MOSRX_ACL_NOT_LOOKED_UP 0xFFFFu
#define MOSRX_ACL_NO_MATCH      0xFFFEu   /* looked up, no rule matched: the default ACCEPT */

/* 0 when n <= MOSRX_ACL_MAX_RULES and every action is one of the two, else
 * -EINVAL (also for rules NULL with n != 0).  Needs no GPU. */
int  mosrx_acl_check(const mosrx_acl_rule *rules, uint32_t n);
/* Validate the rules (mosrx_acl_check) and upload one packed device copy for
 * the context; NULL / 0 clears them.  In effect for launches submitted after it
 * returns; launches already submitted keep the copy they were given (the copies
 * rotate over a pool, and one a launch may have read is rewritten only after
 * those launches drained), as mosrx_fwd_set's. */
int  mosrx_acl_set(mosrx_ctx *c, const mosrx_acl_rule *rules, uint32_t n);
/* Rules installed (0: none). */
uint32_t mosrx_acl_count(const mosrx_ctx *c);
/* The launch over a device-resident batch and its n records of rec_bytes (16 or
 * 8) as a classify call on the same stream left them:
 *   d_hit[n]     u16, 2-byte aligned: the index of the rule that matched,
 *                MOSRX_ACL_NOT_LOOKED_UP or MOSRX_ACL_NO_MATCH
 *   d_counts[MOSRX_ACL_MAX_RULES]  u32, optional: one added per hit (atomic adds:
 *                a sum, so the order does not matter); the caller zeroes it, and
 *                launches into the same array accumulate
 *   d_plan[n]    optional, 8-byte aligned, as mosrx_fwd_plan_dev on the same
 *                stream left it: under forward != 0 the record of a frame whose
 *                rule is DROP becomes the MOSRX_FWD_DROP record above; no other
 *                record is written (forward = 0: none is, the plan stays NONE)
 * One launch; allocates nothing, graph-capturable.  The returns in their order:
 * -EINVAL for a NULL or misaligned pointer or a bad rec_bytes; then -ENOENT with
 * no rules set, whatever n is (as mosrx_fwd_plan_dev without tables); then, for
 * n == 0, 0 with nothing launched. */
int  mosrx_acl_apply_dev(mosrx_ctx *c, const mosrx_batch *b, const void *d_rec, int rec_bytes, mosrx_fwd *d_plan,
                         uint16_t *d_hit, uint32_t *d_counts, void *stream);
/* The batch-queue form: d_hit[nb] (one array per batch; of an empty batch it
 * may be NULL) and d_counts (one array for the queue, or NULL).  mosrx_queue_run
 * then runs one more launch over all of the queue's batches (a workgroup finds
 * its batch in a device-resident table; tiles never straddle batches): with
 * forwarding attached (mosrx_queue_set_fwd / _fwd_desc, before or after this
 * call) between the plan launch and the build launches, amending the attached
 * plan arrays; without, behind the classify launch, with no plan.  The
 * one-launch forwarding form (mosrx_set_fwd_one) plans and builds in one kernel
 * and leaves no place for this launch: a run with rules attached takes the
 * multi-launch path whatever that limit is.  A run with no rules installed is
 * -ENOENT and enqueues nothing.  d_hit NULL detaches. */
int  mosrx_queue_set_acl(mosrx_ctx *c, mosrx_queue *q, uint16_t *const *d_hit, uint32_t *d_counts);
/* The slot arm: the next host group submit on `slot` runs the firewall launch
 * over the group's batches, behind its classify (and steer) launches -- with
 * mosrx_slot_fwd armed too, between the group's plan launch and its descriptor
 * build, amending the group's plan (such a group takes the multi-launch path
 * whatever mosrx_set_fwd_one says: the one launch leaves no place for this
 * one); alone, with no plan.  h_hit[nb]: host arrays of the batches' n u16
 * entries (of an empty batch it may be NULL); h_counts: a host array of
 * MOSRX_ACL_MAX_RULES u32 the group's hits are added to, or NULL.  The hit
 * arrays are written in place for a direct group whose outputs are all pinned
 * and aligned, and copied back otherwise -- the forwarding arm's rule, decided
 * together with it; h_counts is added to in place when it is pinned, else
 * through a copy in and out.  Both are complete when the slot's wait returns.
 * h_hit NULL disarms.  -EBUSY: the slot is in flight; -ENOENT: no rules set (at
 * the arm, and again at the submit); -EINVAL at the submit for a hit array that
 * is NULL or odd of a batch with frames.  Taken by the next group submit on the
 * slot whatever becomes of it. */
int  mosrx_slot_acl(mosrx_ctx *c, int slot, uint16_t *const *h_hit, uint32_t *h_counts);

/* ---- NAT: established flows translated ahead of forwarding --------------------- */
/* What samples/nat does to the TCP frames of a monitored flow (translate_addr,
 * nat.c:91-155): the source address and port become the NAT's (client side), or
 * the destination address and port the client's (server side), and
 * mtcp_setlastpkt recomputes both checksums (mos_api.c:1045-1054, :1107-1122,
 * :1179-1194); ForwardIPPacket then routes the translated daddr (ip_out.c:56-65)
 * and copies the translated packet.  The serial part -- assign_port at a flow's
 * first frame, release_port at its end -- stays on the host, which hands the GPU
 * the bindings in force; the per-frame part is one launch in place of the plan
 * launch (mosrx_fwd_plan_nat_dev) and one behind the byte-ring build
 * (mosrx_nat_patch_rings_dev).
 *
 * The boundary: which frames raise MOS_ON_PKT_IN, and which side a frame is on,
 * is the stream engine's decision behind tcp.c:445.  Here the explicit bindings
 * decide: a frame whose 4-tuple is a binding's client-side key is SNAT, one whose
 * 4-tuple is its server-side key is DNAT, any other eligible frame is a MISS. */
#define MOSRX_NAT_MAX_BINDINGS 64510u   /* the sample's port pool, 1025 .. 65534 (nat.c:244) */
/* One established flow, every field network order as the frame stores it (the
 * raw value of a little-endian host's load). */
typedef struct mosrx_nat_binding {
	uint32_t cli_ip, svr_ip, nat_ip;
	uint16_t cli_port, svr_port, nat_port;
	uint16_t pad;
} mosrx_nat_binding;
enum {
	MOSRX_NAT_NONE = 0,   /* not eligible (non-TCP, ARP, a bad checksum ...): the sample never sees it, mOS forwards it as received */
	MOSRX_NAT_SNAT = 1,   /* client side: saddr / source := addr / port */
	MOSRX_NAT_DNAT = 2,   /* server side: daddr / dest := addr / port */
	MOSRX_NAT_MISS = 3,   /* eligible, no binding: the flow's first frame, for the host to assign a port */
	MOSRX_NAT_HOST = 4    /* eligible, but doff < 5 or a segment under 20 bytes: mtcp_setlastpkt refuses the
	                       * port write (the sample then drops the frame) or writes the check outside the segment */
};
#define MOSRX_NAT_NO_BIND 0xFFFFFFFFu
/* The translation of one frame, 16 bytes.  NONE: all zero.  MISS / HOST: kind,
 * ihl, bind = MOSRX_NAT_NO_BIND, the rest zero. */
typedef struct mosrx_nat_xlat {
	uint32_t addr;        /* the new saddr (SNAT) or daddr (DNAT) */
	uint16_t port;        /* the new source (SNAT) or dest (DNAT) */
	uint16_t ip_check;    /* iph->check after the rewrite */
	uint16_t tcp_check;   /* tcph->check after the rewrite */
	uint8_t  kind;        /* MOSRX_NAT_* */
	uint8_t  ihl;         /* the frame's ihl (5 .. 15) when eligible */
	uint32_t bind;        /* SNAT / DNAT: the binding's index in the installed array */
} mosrx_nat_xlat;
/* The plan kinds of the frames the launch hands to the host: both with tx_len 0,
 * out_ifidx -1, arp_idx 0xFFFF, reserved 0.  Every build sends kinds IP and ETH
 * only, so both fall out of all of them. */
#define MOSRX_FWD_NAT_MISS 7
#define MOSRX_FWD_NAT_HOST 8

/* The lookup table: open addressing, linear probing, a power-of-two number of
 * 32-byte slots, at least 4 per binding (two keys a binding: at most half full).
 * Each binding gives two keys (saddr, daddr, ports = sport | dport << 16):
 *   client side  (cli_ip, svr_ip, cli_port, svr_port) -> SNAT {nat_ip, nat_port}
 *   server side  (svr_ip, nat_ip, svr_port, nat_port) -> DNAT {cli_ip, cli_port}
 * A key lives at slot (mosrx_nat_hash(key) + d) & (slots - 1) for the least d
 * whose slot was free when it went in; kind 0 marks a free slot.  No GPU needed
 * for any of these four. */
typedef struct mosrx_nat_slot {
	uint32_t saddr, daddr, ports;
	uint16_t port;        /* the value: new port, */
	uint8_t  kind;        /*   MOSRX_NAT_SNAT or MOSRX_NAT_DNAT (0: free; MOSRX_NAT_TOMB: deleted, below), */
	uint8_t  pad;
	uint32_t addr;        /*   new address */
	uint32_t bind;        /*   and the binding's index */
	uint32_t reserved[2];
} mosrx_nat_slot;
uint32_t mosrx_nat_hash(uint32_t saddr, uint32_t daddr, uint32_t ports);
/* Slots of the table of n bindings: a power of two, >= 16 and >= 4 * n. */
uint32_t mosrx_nat_slots(uint32_t n);
/* Build the table of n bindings into slots[mosrx_nat_slots(n)] (overwritten
 * whole); *probe (may be NULL): the most slots any key's lookup examines, 0 for
 * n == 0 -- the kernel's loop bound.  -EINVAL as mosrx_nat_check. */
int  mosrx_nat_build(const mosrx_nat_binding *b, uint32_t n, mosrx_nat_slot *slots, uint32_t *probe);
/* 0, or -EINVAL for n over MOSRX_NAT_MAX_BINDINGS, b NULL with n != 0, a zero
 * nat_ip or nat_port, or two keys that are equal -- two client-side keys, two
 * server-side keys, or one of each: a frame must find one answer.  (-ENOMEM:
 * the check builds the table.) */
int  mosrx_nat_check(const mosrx_nat_binding *b, uint32_t n);
/* Validate and build the table on the host and upload it; in effect for
 * launches submitted after it returns.  The device copies rotate over a pool
 * under mosrx_fwd_set's discipline: one a launch may read is rewritten only
 * after that launch drained.  NULL / 0 clears the table, which still counts as
 * set: every eligible frame is then a MISS. */
int  mosrx_nat_set(mosrx_ctx *c, const mosrx_nat_binding *b, uint32_t n);
/* Bindings installed (live ones, after mosrx_nat_update). */
uint32_t mosrx_nat_count(const mosrx_ctx *c);

/* ---- bindings added and removed in place ---- */
/* A slot whose key was deleted: kind MOSRX_NAT_TOMB, every other byte zero.  A
 * lookup steps over it (a free slot would cut the runs of the keys behind it);
 * an insert may reuse it.  Only ever a slot's kind, never an xlat record's. */
#define MOSRX_NAT_TOMB 0xFFu
enum { MOSRX_NAT_OP_ADD = 1, MOSRX_NAT_OP_DEL = 2 };
/* One change: ADD the binding b under the id `bind` (any but MOSRX_NAT_NO_BIND;
 * it is what xlat.bind reports), or DEL the binding b (all of it named; bind is
 * not read). */
typedef struct mosrx_nat_op {
	mosrx_nat_binding b;
	uint32_t op;
	uint32_t bind;
} mosrx_nat_op;
/* The final image of one slot that a list of ops changed. */
typedef struct mosrx_nat_touch {
	uint32_t slot, pad[3];
	mosrx_nat_slot image;
} mosrx_nat_touch;
/* What the arithmetic keeps about a table: its slots (a power of two), its live
 * keys (two a binding), its tombstones, and the loop bound.  Of a table from
 * mosrx_nat_build: {mosrx_nat_slots(n), 2 * n, 0, *probe}. */
typedef struct mosrx_nat_tstate {
	uint32_t slots, keys, tombs, probe;
} mosrx_nat_tstate;
/* Apply ops[0 .. n) in their order to the host table slots[st->slots] and return
 * in touch[4 * n] the final image of every slot that changed: one entry a slot
 * (the last write wins), slots ascending; *ntouch of them.  No GPU needed.
 *   ADD  both keys go in as mosrx_nat_build puts them: the walk from the key's
 *        hash first finds the key absent up to a free slot, then the key takes
 *        the first tombstone that walk passed, or else the free slot.  probe
 *        grows to the new key's distance and never shrinks.
 *   DEL  both keys must be there with one common bind; both slots become
 *        tombstones.
 * A refused call leaves slots and *st byte for byte as they were:
 *   -EINVAL  NULL arguments or a state that is no table's, an op that is neither,
 *            a zero nat_ip or nat_port, bind == MOSRX_NAT_NO_BIND, or more than
 *            MOSRX_NAT_MAX_BINDINGS live bindings;
 *   -EEXIST  an ADD one of whose keys is live;
 *   -ENOENT  a DEL of a binding that is not there;
 *   -ENOSPC  keys + tombs would pass half of the slots (mosrx_nat_build's "at
 *            most half full" with the tombstones counted: what keeps runs short
 *            and every walk ending at a free slot): rebuild. */
int  mosrx_nat_apply(mosrx_nat_slot *slots, mosrx_nat_tstate *st, const mosrx_nat_op *ops, uint32_t n,
                     mosrx_nat_touch *touch, uint32_t *ntouch);
/* The ops applied to the installed table where it lies: mosrx_nat_apply on the
 * context's host mirror of it, then one small launch on `stream` (NULL: the
 * context's own) that stores the changed slots into the installed device copy.
 * ops is dead on return; the device may apply it later, in stream order:
 *   - a launch submitted to that stream before this call reads the old table,
 *     one submitted after it the new one;
 *   - the update waits (on the device, not the host) for every plan-nat launch
 *     the context made on another stream before this call, and for the update
 *     before it;
 *   - launches made on another stream after it are the caller's to order.
 * When the arithmetic answers -ENOSPC the call rebuilds instead: the live
 * bindings and the ops into a fresh table of mosrx_nat_slots(live) slots without
 * tombstones, every bind id kept, installed as mosrx_nat_set installs one (the
 * pool's next copy, a blocking upload, its drain rule).  Either way one call and
 * 0.  Any other refusal (mosrx_nat_apply's, in its terms) leaves the mirror, the
 * device table and the stats as they were and launches nothing.  A context whose
 * table was never set starts from the empty one.  mosrx_nat_set resets the ids to
 * the array's indices.  n == 0: 0, nothing done; n over
 * MOSRX_NAT_UPDATE_MAX_OPS (every port of the pool released and assigned once):
 * -EINVAL.
 * Where the host does wait: for the launch that last read the staging buffer, once
 * four updates are outstanding; in mosrx__drain's place when more callers' streams
 * than the context tracks have run plan-nat; and in the rebuild's blocking upload.
 * Should the launch itself fail in the runtime (-EIO) the mirror is ahead of the
 * device copy until the next mosrx_nat_set; every failure before it leaves both
 * as they were. */
#define MOSRX_NAT_UPDATE_MAX_OPS (2u * MOSRX_NAT_MAX_BINDINGS)
int  mosrx_nat_update(mosrx_ctx *c, const mosrx_nat_op *ops, uint32_t n, void *stream);
typedef struct mosrx_nat_stats {
	uint32_t live, tombs, slots, probe;   /* bindings, tombstones, slots and the loop bound of the installed table */
	uint64_t updates, rebuilds;           /* successful mosrx_nat_update calls; those of them that rebuilt */
} mosrx_nat_stats;
int  mosrx_nat_get_stats(const mosrx_ctx *c, mosrx_nat_stats *out);

/* One launch in place of mosrx_fwd_plan_dev (same arguments, same plan for every
 * frame that is not translated).  A frame is eligible when its reason is TCP_OK,
 * num_msp != 0, the listener flag is off and its IPv4 packet lies inside the
 * capture (the plan's ip_ok).  Its key is read from the frame as the firewall
 * launch reads it (past-the-end bytes read zero) and looked up; d_xlat[i] (16-byte
 * aligned) is written for every frame.  A DNAT frame is routed and ARP-resolved
 * on the translated daddr.  ip_check is ip_fast_csum over the translated header;
 * tcp_check follows from the received check word alone (TCP_OK: the received
 * segment sums to 0xFFFF), TCPCalcChecksum's value bit for bit.  Under forward
 * != 0 a MISS / HOST frame's plan record is the MOSRX_FWD_NAT_* record above.
 * The returns in their order: -EINVAL for a NULL or misaligned pointer (d_xlat
 * to 16, d_plan to 8), a bad rec_bytes or in_ifidx, or a context under
 * skip_tcp_csum (the segment was never summed: no exact incremental check);
 * -ENOENT without forwarding tables, then without mosrx_nat_set; n == 0: 0,
 * nothing launched.  Allocates nothing, graph-capturable. */
int  mosrx_fwd_plan_nat_dev(mosrx_ctx *c, const mosrx_batch *b, const void *d_rec, int rec_bytes, int in_ifidx,
                            mosrx_fwd *d_plan, mosrx_nat_xlat *d_xlat, void *stream);
/* One launch behind mosrx_fwd_build_rings_dev on the same stream, over its
 * outputs: entry e of a ring's written frames (start <= e < start + count;
 * dropped and unwritten entries are never read) whose frame i = d_tx_src[e] is
 * SNAT / DNAT gets, at d_tx_off[e] in d_tx_frames: ip_check at byte 24, addr at
 * 26 (SNAT) or 30 (DNAT), port at 14 + 4 * ihl (SNAT) or two bytes on (DNAT),
 * tcp_check at 14 + 4 * ihl + 16.  n: the batch's frames (the entry arrays' and
 * d_xlat's length).  -EINVAL: NULL or misaligned pointer (d_xlat, d_tx_frames,
 * d_rings to 16, d_tx_off / d_tx_src to 4), nrings outside
 * 1 .. MOSRX_FWD_MAX_NETDEVS.  n == 0 launches nothing.  The descriptor form
 * needs no such launch: there d_xlat[d_tx_src[e]] is the host's descriptor. */
int  mosrx_nat_patch_rings_dev(mosrx_ctx *c, const mosrx_nat_xlat *d_xlat, uint8_t *d_tx_frames,
                               const uint32_t *d_tx_off, const uint32_t *d_tx_src, const mosrx_fwd_ring *d_rings,
                               uint32_t nrings, uint32_t n, void *stream);
/* One record applied to one host frame (from its Ethernet header; NONE / MISS /
 * HOST: untouched): the definition the launch above is tested against. */
void mosrx_nat_patch_frame(uint8_t *frame, const mosrx_nat_xlat *x);
/* The batch-queue form: d_xlat[nb], one array per batch (of an empty batch it may
 * be NULL).  With mosrx_queue_set_fwd attached a run issues classify, (steer,)
 * plan-nat, the build's three launches and the patch; with
 * mosrx_queue_set_fwd_desc plan-nat and the descriptor build's three; each one
 * launch over all batches.  Such a queue takes the multi-launch path whatever
 * mosrx_set_fwd_one says.  -EINVAL with no forwarding attached or with firewall
 * rules attached (here, and again at the run should the attachments have changed),
 * and for a misaligned array.  A run is refused before it enqueues anything with
 * -ENOENT (no bindings set) or -EINVAL (skip_tcp_csum).  NULL detaches. */
int  mosrx_queue_set_nat(mosrx_ctx *c, mosrx_queue *q, mosrx_nat_xlat *const *d_xlat);

/* End-to-end: host frames -> pinned staging -> H2D -> kernel -> D2H -> h_out.
 * Blocks until h_out is filled.  When frames, off and len lie in ONE host
 * block (any order, not overlapping frames_bytes, frames 16-byte aligned
 * within it, gaps under an eighth of the payload + 4 KiB) the batch crosses
 * PCIe in a single copy of that span; otherwise in three (one per array). */
int  mosrx_classify_host(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *h_out);
/* Same, plus the flow hashes into h_fhash[n] (see mosrx_classify_dev_fh). */
int  mosrx_classify_host_fh(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *h_out, uint32_t *h_fhash);
/* Same, with the optional side arrays of mosrx_classify_dev_ex (either may be NULL). */
int  mosrx_classify_host_ex(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *h_out, uint32_t *h_fhash,
                            mosrx_tcpinfo *h_tcpinfo);

/* Asynchronous end-to-end form for pipelining: two slots per context, each
 * with its own stream.  submit enqueues H2D -> kernel -> D2H and returns; wait
 * blocks until that slot's h_out is filled.  The host buffers must stay valid
 * (and unmodified) until the wait returns; pinned buffers (mosrx_host_alloc)
 * make the copies asynchronous. */
#define MOSRX_NSLOT 2
int  mosrx_classify_host_submit(mosrx_ctx *c, int slot, const mosrx_batch *b, mosrx_result *h_out);
int  mosrx_classify_host_wait(mosrx_ctx *c, int slot);
/* Size both slots' device buffers for submits of up to `frames_bytes` of frame
 * buffers (group copies included) and `n` frames, now: without it a slot grows
 * on the first submit that needs more, which synchronises and reallocates (a
 * stall of milliseconds in the middle of traffic).  -EBUSY while a slot runs. */
int  mosrx_classify_host_reserve(mosrx_ctx *c, uint64_t frames_bytes, uint32_t n);
/* 1 when the slot's last submit has completed (its wait would not block) or
 * nothing is outstanding on it, 0 while it runs, -errno on error. */
int  mosrx_classify_host_ready(mosrx_ctx *c, int slot);

/* The same with the pkt_info TCP fields into h_tcpinfo[n] (NULL: none). */
int  mosrx_classify_host_submit_ex(mosrx_ctx *c, int slot, const mosrx_batch *b, mosrx_result *h_out,
                                   mosrx_tcpinfo *h_tcpinfo);

/* A group of `nb` (1..MOSRX_MAX_GROUP) host batches through ONE kernel launch
 * on a pipeline slot (the batch queue of mosrx_queue_*, for batches that start
 * in host memory): the batches' frames and descriptors cross PCIe in as few
 * copies as their layout allows (batches staged back to back in one pinned
 * block, or runs lent one after another by a source, go in one), the kernel
 * classifies all of them, records land in h_out[i] (and pkt_info fields in
 * h_tcpinfo[i] when h_tcpinfo is not NULL).  Wait with
 * mosrx_classify_host_wait; the counters are the group's sum.  Amortises the
 * launch for small batches the way an rx ring of several batches would. */
#define MOSRX_MAX_GROUP 512
int  mosrx_classify_host_group_submit(mosrx_ctx *c, int slot, const mosrx_batch *b, uint32_t nb,
                                      mosrx_result *const *h_out, mosrx_tcpinfo *const *h_tcpinfo);
/* The same, plus the flow-table hash of every frame into h_fhash[i] (NULL: none;
 * see mosrx_classify_dev_fh): the bucket FindStream / HTSearch would compute. */
int  mosrx_classify_host_group_submit_ex(mosrx_ctx *c, int slot, const mosrx_batch *b, uint32_t nb,
                                         mosrx_result *const *h_out, mosrx_tcpinfo *const *h_tcpinfo,
                                         uint32_t *const *h_fhash);
/* The same with 8-byte records (mosrx_result8) into h_out8[i] and, when
 * h_fhash is not NULL, the flow hashes (no pkt_info fields): the group's records are written and copied back at half the bytes
 * (gpu_module_func's cfg.compact, the records an rx loop consumes when it
 * takes pkt_info's lengths from the header, tcp.c:258-270). */
int  mosrx_classify_host_group_submit_c8(mosrx_ctx *c, int slot, const mosrx_batch *b, uint32_t nb,
                                         mosrx_result8 *const *h_out8, uint32_t *const *h_fhash);
/* The same with a BPF set installed: 8-byte records, the flow hashes (NULL:
 * none) and the set's match masks, from one launch of the fused kernel's
 * 8-byte form (or the classify launch + the set per batch while the set has
 * no compiled form). */
int  mosrx_classify_host_group_submit_bpf_c8(mosrx_ctx *c, int slot, const mosrx_batch *b, uint32_t nb,
                                             mosrx_result8 *const *h_out8, uint32_t *const *h_fhash,
                                             uint32_t *const *h_match);
/* The same for a context with a BPF set installed: the records, the flow
 * hashes (h_fhash, NULL: none) and the set's match masks into h_match[i] from
 * ONE launch of the fused classify + BPF queue kernel (the set's compiled
 * form); while the set is still compiling (mosrx_bpf_set_async) or has no
 * compiled form, the classify launch and the set's interpreter kernel per
 * batch, on the slot's stream, same results.  No pkt_info fields with masks. */
int  mosrx_classify_host_group_submit_bpf(mosrx_ctx *c, int slot, const mosrx_batch *b, uint32_t nb,
                                          mosrx_result *const *h_out, uint32_t *const *h_fhash,
                                          uint32_t *const *h_match);

/* Kernel timing on the end-to-end path: with timing on, every submit's kernel
 * launch carries a start / stop event pair its dispatch stamps (the kernel's
 * own duration, as rocprofv3 reports it; events recorded around the two
 * launches of a classify + BPF pair without the fused kernel), and after the
 * wait mosrx_last_kernel_ms gives that device time (-ENODATA if the last
 * waited submit was not timed). */
int  mosrx_set_timing(mosrx_ctx *c, int on);
/* Group submits (mosrx_classify_host_group_submit*) make the per-reason
 * counters of mosrx_last_counters (on, the default) or not (off: no counter
 * atomics in the kernel and no copy back per group; mosrx_last_counters then
 * reads zeros after such a wait).  gpu_module_func turns them off: mOS counts
 * NETSTAT from the records. */
int  mosrx_set_counters(mosrx_ctx *c, int on);
/* Direct groups: a group submit of at most max_frames frames whose frames and
 * descriptors total at most max_bytes (0, the default: none), all of them in
 * pinned memory the library
 * knows (mosrx_host_alloc / mosrx_host_register, or a source's pinned
 * buffers) with 16-byte aligned frame buffers, launches with no copies: the
 * kernel reads them, and the batch table, in place over PCIe, and writes the
 * outputs in place when every output array is pinned too (else it copies
 * them back as usual).  Records are identical either way; a small group skips
 * the copy chain (a blit or SDMA dispatch and a queue handoff per copy), which
 * shortens the group cycle at light load.  mosrx_slot_direct: 1 when the
 * slot's last group submit went direct, 0 if not. */
int  mosrx_set_direct(mosrx_ctx *c, uint64_t max_bytes, uint32_t max_frames);
int  mosrx_slot_direct(mosrx_ctx *c, int slot);
int  mosrx_last_kernel_ms(mosrx_ctx *c, float *ms);

/* Per-reason counters of the last completed end-to-end batch (MOSRX_R_COUNT
 * entries), the NETSTAT rx view of eth_in.c:42-45,80-84. */
int  mosrx_last_counters(mosrx_ctx *c, uint64_t counts[MOSRX_R_COUNT]);

/* Synchronise the context's stream. */
int  mosrx_sync(mosrx_ctx *c);

/* Device memory helpers so callers need no HIP headers. */
int  mosrx_dev_alloc(mosrx_ctx *c, size_t bytes, void **dptr);
int  mosrx_dev_free(mosrx_ctx *c, void *dptr);
/* Pinned (page-locked) host memory: the staging a backend fills from the wire
 * so H2D copies run at full PCIe rate. */
int  mosrx_host_alloc(mosrx_ctx *c, size_t bytes, void **hptr);
int  mosrx_host_free(mosrx_ctx *c, void *hptr);
/* Host memory the caller owns, made known to the library: pinned here
 * (hipHostRegister), or, with MOSRX_HOST_PINNED, already pinned by the caller
 * (hipHostMalloc / hipHostRegister of its own) and only recorded.  Batches and
 * groups whose frames and descriptors lie in one known range cross PCIe in one
 * copy (mosrx_classify_host, the group submits).  Unregister before freeing. */
enum { MOSRX_HOST_PINNED = 1 };
int  mosrx_host_register(mosrx_ctx *c, void *hptr, size_t bytes, int flags);
int  mosrx_host_unregister(mosrx_ctx *c, void *hptr);
int  mosrx_memcpy_h2d(mosrx_ctx *c, void *dst, const void *src, size_t bytes);
int  mosrx_memcpy_d2h(mosrx_ctx *c, void *dst, const void *src, size_t bytes);
/* mosrx_memcpy_h2d done by the CUs instead of the SDMA engine: a kernel reads
 * the pinned host memory over PCIe and writes HBM (src: hipHostMalloc'd or
 * registered memory; -EINVAL otherwise).  Synchronous. */
int  mosrx_memcpy_h2d_pull(mosrx_ctx *c, void *dst, const void *src, size_t bytes);
void *mosrx_stream(mosrx_ctx *c);

/* ---- timing helpers (HIP events on the context stream) -------------------- */
/* Run `iters` classify_dev calls cycling over `nb` resident batches and return
 * the elapsed device time in milliseconds between events recorded on the same
 * stream the kernels run on.  Used by bench.py for the live roofline figure. */
int  mosrx_time_dev(mosrx_ctx *c, const mosrx_batch *b, uint32_t nb,
                    mosrx_result *const *d_out, uint32_t iters, float *ms);
/* Same, with batch i enqueued on stream i % nstreams (1..MOSRX_MAX_STREAMS):
 * independent batches overlap launch and drain, as several rx queues would. */
#define MOSRX_MAX_STREAMS 8
int  mosrx_time_dev_streams(mosrx_ctx *c, const mosrx_batch *b, uint32_t nb,
                            mosrx_result *const *d_out, uint32_t iters, uint32_t nstreams, float *ms);
/* Average duration of one classify kernel over `iters` launches, each bracketed
 * by its own pair of HIP events on the stream it runs on (the roofline figure). */
int  mosrx_time_dev_kernels(mosrx_ctx *c, const mosrx_batch *b, uint32_t nb,
                            mosrx_result *const *d_out, uint32_t iters, float *avg_ms);
/* The same two measurements for any row of the path: `op` over batch i % nb
 * on stream i % nstreams (total_ms), and the average single-launch duration on
 * the context stream (avg_kernel_ms); either pointer may be NULL.  out[i]:
 * records (CLASSIFY, CLASSIFY_FH, CLASSIFY_BPF), match masks (BPF), unused
 * (TX_CSUM, `arg` = its flags); aux[i]: flow hashes (CLASSIFY_FH), match masks
 * (CLASSIFY_BPF). */
enum { MOSRX_OP_CLASSIFY = 0, MOSRX_OP_CLASSIFY_FH = 1, MOSRX_OP_BPF = 2, MOSRX_OP_TX_CSUM = 3,
       MOSRX_OP_CLASSIFY_BPF = 4, MOSRX_OP_CLASSIFY_TI = 5 /* aux[i]: mosrx_tcpinfo side arrays */,
       MOSRX_OP_TX_CHECKS = 6 /* out[i]: mosrx_tx_check records, `arg` the flags */,
       MOSRX_OP_STEER = 7 /* the steer sequence over records already made: out[i] the records of batch i,
                           * aux[i] its idx array, `arg` = rec_bytes (8 or 16); qstart and scratch are the
                           * timing call's own.  Three launches: -ENOTSUP from mosrx_time_op_dispatch */,
       MOSRX_OP_STEER_GATHER = 8 /* MOSRX_OP_STEER with the scatter launch in its gather form: the batch's off / len
                                  * (device resident) are gathered too, into outputs of the timing call's own */,
       MOSRX_OP_STEER_GATHER_SIDE = 9 /* MOSRX_OP_STEER_GATHER in its side form: `arg` = rec_bytes | which << 8, which
                                       * the MOSRX_SIDE_* arrays to gather (0: all three); side sources and outputs
                                       * are the timing call's own */,
       MOSRX_OP_FWD_PLAN = 10 /* the forwarding plan over records already made: out[i] the records of batch i, aux[i]
                               * its mosrx_fwd plan array, `arg` = rec_bytes | in_ifidx << 8 */,
       MOSRX_OP_FWD = 11 /* MOSRX_OP_FWD_PLAN followed by the build (four launches: -ENOTSUP from
                          * mosrx_time_op_dispatch); the TX outputs and scratch are the timing call's own, tx_cap
                          * what the batch's frames need at most */,
       MOSRX_OP_FWD_RINGS = 12 /* MOSRX_OP_FWD_PLAN followed by the ring build (-ENOTSUP from
                                * mosrx_time_op_dispatch); outputs and scratch are the timing call's own, ring_cap
                                * what the batch's frames need at most, nrings the tables' num_netdevs */,
       MOSRX_OP_FWD_DESC = 13 /* MOSRX_OP_FWD_PLAN followed by the descriptor form of the ring build (-ENOTSUP from
                               * mosrx_time_op_dispatch); outputs and scratch are the timing call's own, nrings the
                               * tables' num_netdevs */,
       MOSRX_OP_ACL = 14 /* the firewall launch (mosrx_acl_apply_dev) over records already made: out[i] the records
                          * of batch i, aux[i] its u16 hit array, `arg` = rec_bytes; no plan and no counts.  Not a
                          * kernel of the classify object: -ENOTSUP from mosrx_time_op_dispatch */,
       MOSRX_OP_FWD_NAT = 15 /* plan-nat, the ring build and the patch (mosrx_fwd_plan_nat_dev,
                              * mosrx_fwd_build_rings_dev, mosrx_nat_patch_rings_dev) over records already made:
                              * out / aux / `arg` as MOSRX_OP_FWD_RINGS; the xlat array is the timing call's own.
                              * -ENOTSUP from mosrx_time_op_dispatch */ };
int  mosrx_time_op(mosrx_ctx *c, int op, int arg, const mosrx_batch *b, uint32_t nb, void *const *out,
                   void *const *aux, uint32_t iters, uint32_t nstreams, float *total_ms, float *avg_kernel_ms);
/* The kernel's own duration, averaged over `iters` back-to-back launches on
 * the context stream: each launch carries a start / stop event pair that the
 * dispatch itself stamps (hipExtLaunchKernel), so the gap between dispatches
 * is not counted -- the duration rocprofv3's kernel trace reports.  -ENOTSUP
 * for an operation that is not one kernel launch (the BPF rows). */
int  mosrx_time_op_dispatch(mosrx_ctx *c, int op, int arg, const mosrx_batch *b, uint32_t nb, void *const *out,
                            void *const *aux, uint32_t iters, float *avg_ms);
int  mosrx_time_queue_dispatch(mosrx_ctx *c, mosrx_queue *const *q, uint32_t nq, uint32_t iters, float *avg_ms);
/* The device's streaming-read ceiling: `iters` coalesced 16-byte-load passes
 * cycling over `nbuf` buffers of `bytes` each (sized past the 256 MiB Infinity
 * Cache), in GB/s.  The roofline figure next to the 8 TB/s spec peak. */
int  mosrx_probe_read_bw(mosrx_ctx *c, uint64_t bytes, uint32_t nbuf, uint32_t iters, float *gbps);
/* The stamp's own floor: the average dispatch-stamped duration (as
 * mosrx_time_op_dispatch measures it) of an empty kernel with the grid a
 * classify launch of `b` would have.  A short launch's stamped figure is
 * stated against it (the stamp reads ~4 us for a kernel that does nothing,
 * rocprofv3's trace 1.5-2.9 us).  Diagnostic; no mOS counterpart. */
int  mosrx_probe_stamp_floor(mosrx_ctx *c, const mosrx_batch *b, uint32_t iters, float *avg_ms);
/* hipDeviceSynchronize on the context's device. */
int  mosrx_device_sync(mosrx_ctx *c);
/* Same, end-to-end from host buffers through pinned staging, double-buffered. */
int  mosrx_time_host(mosrx_ctx *c, const mosrx_batch *b, uint32_t nb,
                     mosrx_result *const *h_out, uint32_t iters, float *ms);

/* ---- batched BPF ---------------------------------------- */
/* mOS evaluates classic-BPF programs per frame: raw-monitor filters on the
 * whole frame (ip_in.c:56-63) and stream SYN / orphan filters on the IP
 * datagram (tcp.c:42-56, 486-496), each through EVAL_BPFFILTER ->
 * sfbpf_filter(insns, p, len, len) (include/bpf/sfbpf.h:84,
 * bpf/sf_bpf_filter.c:214-536).  Programs still come from mOS's own compiler
 * (SET_BPFFILTER -> sfbpf_compile, sfbpf.h:83); the GPU runs the batched
 * evaluation of up to 32 of them over a batch and returns one match bitmask
 * per frame. */
typedef struct mosrx_bpf_insn {   /* layout of struct sfbpf_insn (include/bpf/sfbpf.h:174-179) */
	uint16_t code;
	uint8_t  jt;
	uint8_t  jf;
	uint32_t k;
} mosrx_bpf_insn;

enum {
	MOSRX_BPF_LEN_FRAME = 0,  /* wirelen = buflen = caplen (raw monitor: ethh, eth_len) */
	MOSRX_BPF_LEN_IP    = 1,  /* wirelen = buflen = 14 + ip tot_len (SYN/orphan filters);
	                           * evaluated on IPv4 frames whose datagram lies inside caplen, else 0 */
};
#define MOSRX_BPF_MAX_PROGS 32
#define MOSRX_BPF_MAX_INSNS 4096   /* total over all programs of a set */

typedef struct mosrx_bpf_prog {
	const mosrx_bpf_insn *insns;   /* NULL or len 0: no filter, matches every frame (sfbpf_filter(NULL) = ~0) */
	uint32_t              len;     /* bf_len */
	int32_t               len_mode;/* MOSRX_BPF_LEN_* */
} mosrx_bpf_prog;

/* The admission check of mosrx_bpf_set for one program (no GPU needed):
 * 0 or -EINVAL.  Besides sfbpf_validate's rules it rejects the absolute word /
 * halfword loads whose offset wraps sfbpf_filter's int bounds check (k of
 * 0xFFFFFFFC.. for a word, 0xFFFFFFFE.. for a halfword: the reference reads
 * before the frame).  The indexed loads cannot be checked at set time: where
 * X + k wraps into those ranges the reference reads before the frame
 * (undefined) and the GPU returns 0, as sfbpf_filter does for every other
 * out-of-bounds offset. */
int  mosrx_bpf_check(const mosrx_bpf_insn *insns, uint32_t len);
/* Install a program set on the context (host arrays, copied).  Each program
 * must pass sfbpf_validate (sf_bpf_filter.c:548-691) and, beyond it, use only
 * opcodes sfbpf_filter executes (others abort() there) with jump targets that
 * stay forward in 64-bit pointer arithmetic; otherwise -EINVAL, as
 * SET_BPFFILTER failing makes mtcp_bind_monitor_filter return EINVAL
 * (mos_api.c:127-155).  nprog = 0 clears the set. */
int  mosrx_bpf_set(mosrx_ctx *c, const mosrx_bpf_prog *progs, uint32_t nprog);
/* The same without waiting for the compiled form: the set is admitted,
 * staged and in effect when this returns (microseconds; no device-wide
 * synchronisation), evaluated by the interpreter kernel until the context's
 * compile thread has built and loaded its kernels with hipRTC, which replace
 * it at the next launch (a set seen before is taken from the cache at once).
 * Results are the same on either engine.  mosrx_bpf_wait blocks until the
 * installed set's compiled form is in (or failed: the interpreter stays);
 * mosrx_bpf_pending is 1 while its compile is outstanding. */
int  mosrx_bpf_set_async(mosrx_ctx *c, const mosrx_bpf_prog *progs, uint32_t nprog);
int  mosrx_bpf_wait(mosrx_ctx *c);
int  mosrx_bpf_pending(mosrx_ctx *c);
/* Evaluation engine of the next mosrx_bpf_set.  JIT (default): the set is
 * translated to one straight-line gfx950 kernel and compiled with hipRTC at
 * set time (cached per context); INTERP: the uniform-pc interpreter kernel.
 * Both run on the GPU with the same results; env MOSRX_BPF_ENGINE=0 selects
 * INTERP at open.  mosrx_bpf_engine() reports the engine of the installed set
 * (INTERP when the JIT could not compile; mosrx_bpf_jit_log() says why). */
enum { MOSRX_BPF_ENGINE_INTERP = 0, MOSRX_BPF_ENGINE_JIT = 1 };
int  mosrx_bpf_set_engine(mosrx_ctx *c, int engine);
int  mosrx_bpf_engine(const mosrx_ctx *c);
const char *mosrx_bpf_jit_log(const mosrx_ctx *c);
/* The generated kernel source of a program set (no GPU needed; free() it). */
int  mosrx_bpf_jit_source(const mosrx_bpf_prog *progs, uint32_t nprog, char **src);
/* The generated hook of the fused classify + BPF kernel: the set as the
 * device function the header wave calls on its window (free() it). */
int  mosrx_bpf_jit_hook_source(const mosrx_bpf_prog *progs, uint32_t nprog, char **src);
/* Generate and compile a program set with hipRTC for gfx950 without loading
 * it (no GPU needed): 0 and the code-object size, or -errno and the log. */
int  mosrx_bpf_jit_compile(const mosrx_bpf_prog *progs, uint32_t nprog, char *log, size_t logsz,
                           size_t *code_size);
/* Same for the fused classify + BPF kernel (the set inlined into the
 * classification kernel's header wave). */
int  mosrx_bpf_jit_compile_fused(const mosrx_bpf_prog *progs, uint32_t nprog, char *log, size_t logsz,
                                 size_t *code_size);
/* Classification (as mosrx_classify_dev) and the installed BPF set (as
 * mosrx_bpf_dev) in ONE pass over the frames: with the JIT engine the set is
 * compiled into the classify kernel, whose header wave evaluates it on the
 * bytes it already holds; otherwise two launches, same results.
 * mosrx_bpf_fused() = 1 when the installed set has the fused kernel. */
int  mosrx_classify_bpf_dev(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *d_out, uint32_t *d_match,
                            void *stream);
int  mosrx_bpf_fused(const mosrx_ctx *c);
/* The same from host memory: H2D, the one-pass kernel, D2H of records and
 * masks (blocking, or submit/wait on a pipeline slot like mosrx_classify_host). */
int  mosrx_classify_bpf_host(mosrx_ctx *c, const mosrx_batch *b, mosrx_result *h_out, uint32_t *h_match);
int  mosrx_classify_bpf_host_submit(mosrx_ctx *c, int slot, const mosrx_batch *b, mosrx_result *h_out,
                                    uint32_t *h_match);
/* Device-resident evaluation: d_match[i] bit j = (sfbpf_filter(prog j, frame i) != 0). */
int  mosrx_bpf_dev(mosrx_ctx *c, const mosrx_batch *b, uint32_t *d_match, void *stream);
/* End-to-end from host memory (blocking). */
int  mosrx_bpf_host(mosrx_ctx *c, const mosrx_batch *b, uint32_t *h_match);

/* ---- TX checksum generation ---------------------------- */
/* The checksum rewrite mOS applies to a frame before it goes out again:
 * mtcp_setlastpkt with MOS_UPDATE_IP_CHKSUM / MOS_UPDATE_TCP_CHKSUM
 * (mos_api.c:1177-1193): iph->check = 0, iph->check = ip_fast_csum(iph, ihl);
 * tcph->check = 0, tcph->check = TCPCalcChecksum(tcph, tot_len - ihl*4, saddr,
 * daddr) -- the same arithmetic as the S/W fallback of ip_out.c:169-174 and
 * tcp_out.c:207-218.  Flags use mos_api.h:107-108's values.  Frames are
 * rewritten IN PLACE (b->frames is written through); frames must not overlap.
 * IP check: IPv4 frames with ihl >= 5 and the datagram inside the capture.
 * TCP check: those of them with protocol 6 and tot_len >= (ihl + doff) * 4.
 * Other frames are left untouched. */
#define MOSRX_TX_IP_CSUM  (1 << 4)   /* MOS_UPDATE_IP_CHKSUM */
#define MOSRX_TX_TCP_CSUM (1 << 5)   /* MOS_UPDATE_TCP_CHKSUM */
int  mosrx_tx_csum_dev(mosrx_ctx *c, const mosrx_batch *b, int flags, void *stream);
/* The same checks without touching the frames: one 8-byte record per frame
 * into d_checks (8-byte aligned, b->n of them).  `what` bit 0: ip_check is the
 * frame's new iph->check (little-endian u16 at frame byte 24), bit 1:
 * tcp_check its new tcph->check (at frame byte 14 + 4 * ihl + 16); frames the
 * rewrite would leave untouched have what = 0.  For a consumer that writes
 * the words itself (mosrx_tx_csum_host does, on the host).  Same checks as
 * mtcp_setlastpkt's MOS_UPDATE_IP_CHKSUM / MOS_UPDATE_TCP_CHKSUM
 * (core/src/mos_api.c:1177-1193) and the S/W paths of ip_out.c:169-174,
 * tcp_out.c:207-218. */
typedef struct mosrx_tx_check {
	uint16_t ip_check;
	uint16_t tcp_check;
	uint8_t  what;
	uint8_t  ihl;
	uint16_t pad;
} mosrx_tx_check;
int  mosrx_tx_csum_dev_checks(mosrx_ctx *c, const mosrx_batch *b, int flags, mosrx_tx_check *d_checks,
                              void *stream);
/* End-to-end from host memory (blocking): the frames cross PCIe once, the
 * check records come back and are written into b->frames. */
int  mosrx_tx_csum_host(mosrx_ctx *c, const mosrx_batch *b, int flags);

/* ---- RSS helpers (host-side table build; the hash itself runs on the GPU) -- */
/* Toeplitz nibble tables: 24 tables x 16 u32 for the 12-byte tuple
 * saddr|daddr|sport|dport (wire order).  Built from the key cache of
 * BuildKeyCache (util.c:27-58). */
int  mosrx_rss_tables(const uint8_t *key, uint32_t key_len, uint32_t tables[24 * 16]);

int  mosrx_abi_version(void);
const char *mosrx_strerror(int err);

#ifdef __cplusplus
}
#endif
#endif /* MOSRX_H */
