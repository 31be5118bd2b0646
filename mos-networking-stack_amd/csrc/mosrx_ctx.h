/*
 * mosrx_ctx.h — host-side context layout shared by the C host files
 * (mosrx_api.c, bpf_api.c, fwd_api.c, acl_api.c, nat_api.c).  Not part of the ABI.
 */
#ifndef MOSRX_CTX_H
#define MOSRX_CTX_H

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "mosrx_internal.h"
#include "mosrx_steer.h"
#include "mosrx_fwd.h"
#include "mosrx_acl.h"
#include "mosrx_nat.h"

#define HIPCHK(x) do { if ((x) != hipSuccess) return -EIO; } while (0)

#define MOSRX_BPF_JIT_CACHE 16   /* compiled program sets kept per context */
#define MOSRX_BPF_POOL 8         /* device buffers the interpreter's instructions rotate over */
#define MOSRX_FWD_POOL 4         /* device copies the forwarding tables rotate over */
#define MOSRX_ACL_POOL 4         /* device copies the firewall rules rotate over */
#define MOSRX_NAT_POOL 4         /* device copies the NAT lookup table rotates over */

/* The fused classify + BPF kernels of a compiled set (bpf_jit.c k_fused_main):
 * one batch as the stream tile (non-temporal / cached tails) or the SMALL tile,
 * the same three over a batch queue, and those three with 8-byte records. */
#define MOSRX_BPF_NFUSED 9
enum { FU_S = 0, FU_SR = 1, FU_M = 2, FU_QS = 3, FU_QSR = 4, FU_QM = 5, FU_QS8 = 6, FU_QSR8 = 7, FU_QM8 = 8 };
struct mosrx_jit_entry {
	uint64_t key;                          /* set_hash of the set */
	hipModule_t mod, fmod;
	hipFunction_t fn;                      /* the set's own kernel; NULL: the compile failed */
	hipFunction_t fu[MOSRX_BPF_NFUSED];    /* fused kernels; NULL: none (two launches) */
};
struct mosrx_bpf_worker;                   /* the context's compile thread (bpf_jit.c) */

/* pipeline slots for the end-to-end path (double-buffered H2D | kernel | D2H) */
#define NSLOT MOSRX_NSLOT

struct slot {
	uint8_t *d_frames;
	uint32_t *d_off;
	uint16_t *d_len;
	mosrx_result *d_res;
	uint32_t *d_fh;
	mosrx_tcpinfo *d_ti;
	uint32_t *d_match;         /* BPF match masks (the group submit with a set installed) */
	uint32_t *d_cnt;
	uint64_t cap_frames;
	uint32_t cap_n;
	hipStream_t stream;
	hipEvent_t done;
	uint32_t *h_cnt;   /* MOSRX_CNT_WORDS, pinned: a D2H copy into pageable memory blocks the host */
	/* The counters only grow: a submit adds to d_cnt and copies it back into
	 * h_cnt, and the wait takes the batch's counts as h_cnt - h_prev (u32
	 * arithmetic, so wrapping is harmless), then keeps h_cnt as h_prev.  No
	 * memset (a blit kernel and a dependent dispatch) per submit; cnt_dirty: the
	 * device words are not h_prev (first use, a submit that failed after its
	 * launch), and the next submit zeroes both. */
	uint32_t *h_prev;
	int cnt_dirty;
	int counted;               /* the last submit made reason counts (mosrx_set_counters) */
	hipEvent_t kev0, kev1;     /* around the kernel of the last submit (when the context times) */
	mosrx_qdesc *h_qdesc;      /* MOSRX_MAX_GROUP, pinned: a group's batch table */
	mosrx_tx_check *h_txc;     /* pinned: the TX pass's check records (mosrx_tx_csum_host), h_txc_n of them */
	uint32_t h_txc_n;
	mosrx_qdesc *d_qdesc;
	const mosrx_qdesc *hq_dev; /* h_qdesc's device address (a direct group's batch table), NULL: none */
	int direct;                /* the last group submit was direct (mosrx_set_direct) */
	/* queue steering of a group (mosrx_slot_steer): the armed outputs (NULL:
	 * none; taken by the next group submit), the group's batch table (pinned,
	 * copied to d_sdesc per armed submit), and the buffers slot_reserve sizes
	 * with the rest: idx for cap_n frames, a histogram row per tile a group of
	 * cap_n frames in MOSRX_MAX_GROUP batches can have, qstart per batch */
	uint32_t *const *steer_idx, *const *steer_qstart;
	mosrx_sdesc *h_sdesc, *d_sdesc;
	uint32_t *d_sidx, *d_shist, *d_sqstart;
	/* ... and of its queue-major gather (mosrx_slot_steer_gather): the armed
	 * outputs (steer_qrec NULL: a plain steer; steer_qoff / steer_qlen NULL:
	 * records only), the gather table parallel to h_sdesc / d_sdesc, and the
	 * slot's own records, offsets and lengths for cap_n frames */
	void *const *steer_qrec;
	uint32_t *const *steer_qoff;
	uint16_t *const *steer_qlen;
	mosrx_gdesc *h_gdesc, *d_gdesc;
	uint8_t *d_sqrec;
	uint32_t *d_sqoff;
	uint16_t *d_sqlen;
	/* ... and of the gather's side form (mosrx_slot_steer_gather_side): the
	 * armed outputs (each NULL: that array is not gathered), the side table
	 * parallel to the other two, and the slot's own arrays for cap_n frames */
	uint32_t *const *steer_qfhash, *const *steer_qmatch;
	mosrx_tcpinfo *const *steer_qtcpinfo;
	mosrx_xdesc *h_xdesc, *d_xdesc;
	uint32_t *d_sqfh, *d_sqmt;
	mosrx_tcpinfo *d_sqti;
	/* forwarding of a group (mosrx_slot_fwd): the armed outputs (fwd_armed; taken
	 * by the next group submit), the two batch tables of the descriptor queue
	 * form (pinned, copied to the device per armed submit), the ring rows of
	 * every batch, and the buffers slot_reserve sizes with the rest: plan and
	 * entries for cap_n frames, a scratch row per ring and tile a group of cap_n
	 * frames in MOSRX_MAX_GROUP batches can have */
	mosrx_slot_fwd_out fwd;
	int fwd_armed;
	mosrx_fdesc *h_fdesc, *d_fdesc;
	mosrx_ddesc *h_ddesc, *d_ddesc;
	mosrx_fwd_ring *d_frings;
	mosrx_fwd *d_fplan;
	uint32_t *d_ftsrc, *d_ftmac, *d_fscr;
	uint16_t *d_ftlen;
	/* the firewall launch of a group (mosrx_slot_acl): the armed outputs (acl_armed;
	 * taken by the next group submit), the group's batch table (pinned, copied to
	 * the device per armed submit), hits for cap_n frames and one counts array */
	uint16_t *const *acl_hit;
	uint32_t *acl_counts;
	int acl_armed;
	mosrx_adesc *h_adesc, *d_adesc;
	uint16_t *d_ahit;
	uint32_t *d_acnt;
	int timed;
	int busy;
};

struct mosrx_ctx {
	int device;
	hipStream_t stream;
	mosrx_params params;
	uint32_t kflags;
	uint32_t *d_tables;
	struct slot slot[NSLOT];
	uint32_t h_cnt[MOSRX_R_COUNT];   /* counters of the last waited batch */
	hipEvent_t ev0, ev1;
	int variant;                     /* kernel cache-policy variant (mosrx_set_variant) */
	mosrx_bpf_insn *d_bpf;           /* installed BPF programs (MOSRX_BPF_MAX_INSNS), NULL until set:
	                                  * one of the pool's buffers */
	mosrx_bpf_insn *d_bpf_pool[MOSRX_BPF_POOL];
	int bpf_pool_used[MOSRX_BPF_POOL];   /* a launch may have read it since it was written */
	uint32_t bpf_pool_next;
	mosrx_bparams bpf;               /* program table of the installed set */
	hipFunction_t bpf_fn;            /* compiled form of the installed set (bpf_jit.c), NULL: interpreter */
	int bpf_engine_req;              /* MOSRX_BPF_ENGINE_* for the next mosrx_bpf_set */
	char bpf_jit_log[512];           /* hipRTC log of the last failed compile */
	hipFunction_t bpf_fu[MOSRX_BPF_NFUSED];   /* fused classify + BPF kernels, NULL: none */
	struct mosrx_jit_entry jit[MOSRX_BPF_JIT_CACHE];
	uint32_t njit;
	uint64_t bpf_key;                /* set_hash of the installed set */
	int bpf_pending;                 /* its compile is outstanding (the interpreter runs it meanwhile) */
	struct mosrx_bpf_worker *bw;
	hipStream_t xs[MOSRX_MAX_STREAMS];   /* timing streams (mosrx_time_op), created on first use */
	hipEvent_t xdone[MOSRX_MAX_STREAMS];
	uint32_t nxs;
	/* callers' streams a launch reading the installed set went to since the last
	 * drain, each with an event recorded after that launch (mosrx__note_stream);
	 * foreign_streams: more of them than the table holds, so the drain falls back
	 * to a device-wide sync */
#define MOSRX_FOREIGN 8
	hipStream_t fstream[MOSRX_FOREIGN];
	hipEvent_t fev[MOSRX_FOREIGN];
	uint32_t nfs;
	int foreign_streams;
	int timing;                      /* record kernel events on the end-to-end path (mosrx_set_timing) */
	int no_counters;                 /* group submits make no reason counts (mosrx_set_counters) */
	uint64_t direct_max;             /* largest direct group, input bytes (mosrx_set_direct); 0: none */
	uint32_t direct_frames;          /*   and its most frames */
	float last_kernel_ms;            /* kernel time of the last waited submit, -1 if not timed */
	/* MOSRX_OP_STEER's own qstart + scratch, one block of steer_tmp_stride bytes
	 * per timing stream and one for the context stream (mosrx_time_op) */
	uint8_t *steer_tmp;
	size_t steer_tmp_stride, steer_tmp_bytes;
	size_t steer_tmp_scratch;        /*   the scratch part of a block, and the frames its gather part holds */
	uint32_t steer_tmp_n;
	uint32_t steer_one;              /* batches of at most this many frames steer in one launch (mosrx_set_steer_one); 0: off */
	uint64_t steer_one_count;        /*   steer launches that did */
	/* forwarding (mosrx_fwd_set): the installed tables' device copy (NULL: none),
	 * one of a pool under the BPF instruction buffers' discipline -- each set goes
	 * to the next buffer, and a buffer a launch may have read is rewritten only
	 * after mosrx__drain */
	mosrx_fwd_dev *d_fwd;
	mosrx_fwd_dev *d_fwd_pool[MOSRX_FWD_POOL];
	int fwd_pool_used[MOSRX_FWD_POOL];
	uint32_t fwd_pool_next;
	uint32_t fwd_listener;           /* mosrx_fwd_set_listener */
	uint32_t fwd_num_netdevs;        /* the installed tables' num_netdevs (the ring build's least nrings) */
	uint32_t fwd_one;                /* batches of at most this many frames are planned and built in one launch (mosrx_set_fwd_one); 0: off */
	uint64_t fwd_one_count;          /*   forwarding launches that were */
	/* MOSRX_OP_FWD's / MOSRX_OP_FWD_RINGS' own TX outputs + scratch, one block of
	 * fwd_tmp_stride bytes per timing stream and one for the context stream
	 * (mosrx_time_op); fwd_tmp_rings rings of fwd_tmp_cap bytes (MOSRX_OP_FWD: 1) */
	uint8_t *fwd_tmp;
	size_t fwd_tmp_stride, fwd_tmp_bytes, fwd_tmp_cap;
	uint32_t fwd_tmp_n, fwd_tmp_rings;
	/* firewall rules (mosrx_acl_set): the installed rules' device copy (NULL:
	 * none), one of a pool under the forwarding tables' discipline */
	mosrx_acl_dev *d_acl;
	mosrx_acl_dev *d_acl_pool[MOSRX_ACL_POOL];
	int acl_pool_used[MOSRX_ACL_POOL];
	uint32_t acl_pool_next;
	uint32_t acl_n;                  /* the installed rules' count */
	/* NAT bindings (mosrx_nat_set): the installed lookup table's device copy (NULL:
	 * never set), one of a pool under the forwarding tables' discipline; a copy
	 * grows when a table needs more slots than it has */
	mosrx_nat_slot *d_nat;
	mosrx_nat_slot *d_nat_pool[MOSRX_NAT_POOL];
	size_t nat_pool_bytes[MOSRX_NAT_POOL];
	int nat_pool_used[MOSRX_NAT_POOL];
	uint32_t nat_pool_next;
	uint32_t nat_n, nat_mask, nat_probe;   /* the installed table: bindings, slots - 1, the longest probe run */
	/* ... and its host mirror (mosrx_nat_update): the table as it was built and
	 * changed since, which also holds the live bindings and their ids */
	mosrx_nat_slot *nat_h;
	mosrx_nat_tstate nat_st;
	uint64_t nat_updates, nat_rebuilds;
	/* the touch lists of the last MOSRX_NAT_STAGE updates, pinned and read by the
	 * update launch where they lie (d: the device address); ev is recorded behind
	 * that launch, and a buffer is written again only after its event (busy) */
#define MOSRX_NAT_STAGE 4
	struct {
		mosrx_nat_touch *h;
		const mosrx_nat_touch *d;
		uint32_t cap;
		hipEvent_t ev;
		hipStream_t stream;
		int busy;
	} nat_stage[MOSRX_NAT_STAGE];
	uint32_t nat_stage_next;
	/* the context's own streams a plan-nat launch went to since the last update
	 * (bit 0: stream, 1 ..: the slots', then xs[]), and an event for each: the
	 * update's stream waits for them (callers' streams: fev[], above) */
#define MOSRX_NAT_OWN (1 + NSLOT + MOSRX_MAX_STREAMS)
	uint32_t nat_own_mask;
	hipEvent_t nat_own_ev[MOSRX_NAT_OWN];
};

/* ---- batch queue (one launch over many resident batches) ---- */
struct mosrx_queue {
	mosrx_qdesc *d_desc;
	mosrx_qdesc *h_desc;   /* host copy: the per-batch BPF launches of a queue with masks */
	uint32_t nb;
	uint32_t total_tiles;
	uint32_t tpb;   /* tiles per batch if uniform, else 0 */
	int tile;
	uint64_t bytes, n;   /* frame bytes and frames of all batches (tail policy) */
	int compact;         /* 8-byte records */
	int uni;             /* some batch carries a layout hint */
	int match;           /* the descriptors' bmatch: the installed BPF set's masks */
	uint32_t **d_match;  /* per batch (the non-fused form) */
	/* queue steering (mosrx_queue_set_steer): the batches' steer table and the
	 * histogram rows, allocated at the first attach; steer: outputs attached */
	mosrx_sdesc *d_sdesc;
	uint32_t *d_shist;
	uint32_t steer_tiles;
	uint32_t steer_maxn;   /* the largest batch, kept at attach: a run takes the one-launch form by it */
	int steer;
	/* its gather form (mosrx_queue_set_steer_gather): the table parallel to
	 * d_sdesc; gather: the scatter pass of a run is the gather form */
	mosrx_gdesc *d_gdesc;
	int gather;
	/* ... and its side form (mosrx_queue_set_steer_gather_side), the third table */
	mosrx_xdesc *d_xdesc;
	int side;
	/* forwarding (mosrx_queue_set_fwd): the batches' table and the build's
	 * scratch rows, allocated at the first attach that needs them; fwd: a plan
	 * attached, fwd_build: with the ring build */
	mosrx_fdesc *d_fdesc;
	uint32_t *d_fscratch;
	size_t fscratch_rows;
	uint32_t fwd_tiles, fwd_nrings, fwd_cap_units;
	int fwd, fwd_build;
	/* its descriptor form (mosrx_queue_set_fwd_desc): the store launch's table,
	 * parallel to d_fdesc; fwd_desc: attached (then fwd is set, fwd_build is not) */
	mosrx_ddesc *d_ddesc;
	int fwd_desc;
	uint32_t fwd_maxn;   /*   its largest batch: what mosrx_set_fwd_one's limit is held against */
	/* firewall rules (mosrx_queue_set_acl): the batches' table, allocated at the
	 * first attach, its tile count (the forwarding tables' tile_base[], built the
	 * same way) and the queue's counts array (NULL: none); acl: attached */
	mosrx_adesc *d_adesc;
	uint32_t *acl_counts;
	uint32_t acl_tiles;
	int acl;
	/* NAT (mosrx_queue_set_nat): the batches' xlat arrays, a device table parallel
	 * to d_fdesc allocated at the first attach; nat: attached */
	mosrx_nat_xlat **d_nxtab;
	int nat;
};

int mosrx__check_batch(const mosrx_batch *b, int dev);
void *mosrx__host_dev_of(const void *p, uint64_t len, int device);
int mosrx__bpf_jit_request(mosrx_ctx *c, const mosrx_bpf_insn *insns);
int mosrx__bpf_jit_wait(mosrx_ctx *c);
void mosrx__bpf_poll(mosrx_ctx *c);
int mosrx__bpf_fused_queue_launch(mosrx_ctx *c, const mosrx_qparams *qp, uint32_t total_tiles, int small,
                                  int variant, hipStream_t s);
/* The installed set's standalone kernel (compiled, else the interpreter) over a
 * device-resident batch, match masks into match[n]. */
int mosrx__bpf_launch_dev(mosrx_ctx *c, const uint8_t *frames, uint64_t frames_bytes, const uint32_t *off,
                          const uint16_t *len, uint32_t n, uint32_t *match, hipStream_t s);
int mosrx__bpf_jit_launch(mosrx_ctx *c, const mosrx_bparams *bp, hipStream_t s);
int mosrx__bpf_jit_source(const mosrx_bpf_insn *insns, const mosrx_bparams *t, char **out);
void mosrx__bpf_jit_free(mosrx_ctx *c);
int mosrx__bpf_jit_compile(const char *src, char *log, size_t logsz, size_t *code_size);
int mosrx__bpf_jit_compile_fused(const mosrx_bpf_insn *insns, const mosrx_bparams *t, char *log, size_t logsz,
                                 size_t *code_size);
int mosrx__bpf_jit_hook_source(const mosrx_bpf_insn *insns, const mosrx_bparams *t, char **out);
int mosrx__bpf_fused_launch(mosrx_ctx *c, const mosrx_kparams *kp, int small, hipStream_t s);
int mosrx__slot_reserve(mosrx_ctx *c, struct slot *s, uint64_t frames_bytes, uint32_t n);
/* A launch that reads the installed BPF set (its staged instructions or its
 * compiled module) was just made on stream s: when s is not one of the
 * context's own streams (a caller's stream), an event recorded on s after it
 * lets mosrx__drain wait for exactly that work. */
void mosrx__note_stream(mosrx_ctx *c, hipStream_t s);
/* Every launch that may still read a staged instruction buffer or a compiled
 * module has finished: the context's own streams synchronised, and the events
 * noted on callers' streams since the last drain (the whole device only when
 * more streams were used than the table holds).  Before a buffer is rewritten
 * or a module unloaded. */
int mosrx__drain(mosrx_ctx *c);

/* The variant a launch of `n` frames in `bytes` runs: the context's, with the
 * tail loads cached instead of non-temporal for batches of small frames when
 * the context runs the library default (mosrx_api.c). */
int mosrx__tail_variant(const mosrx_ctx *c, uint64_t bytes, uint64_t n);

/* ---- forwarding's host side (fwd_api.c), as mosrx_api.c's flows reach it ---- */

/* What an armed group (mosrx_slot_fwd) needs of the context, at the arm and
 * again at the submit, since the tables may change in between: -ENOENT with no
 * tables installed, -EINVAL with fewer rings than the tables have netdevs. */
int mosrx__fwd_group_check(const mosrx_ctx *c, const mosrx_slot_fwd_out *o);
/* ... and of batch i's outputs, n its frame count: -EINVAL for an input netdev
 * out of range, ring rows that are NULL or not 4-byte aligned, or, of a batch
 * with frames, an array that is NULL or not aligned to its entries. */
int mosrx__fwd_group_check_batch(const mosrx_slot_fwd_out *o, uint32_t i, uint32_t n);
/* A group without a frame launches nothing: its nb batches' ring rows, zeroed
 * on the host, are its whole forwarding output. */
void mosrx__fwd_group_empty(const mosrx_slot_fwd_out *o, uint32_t nb);
/* The device addresses of an armed group's forwarding outputs, when every one
 * of them is pinned and aligned to its stores (ring rows: 16 bytes): into the
 * slot's two forwarding tables, fd and dd.  1: all are there and the launches
 * may write in place; 0: the group copies back from the slot's own buffers. */
int mosrx__fwd_group_outputs(int device, const mosrx_batch *b, uint32_t nb, const mosrx_slot_fwd_out *o, mosrx_fdesc *fd,
                             mosrx_ddesc *dd);
/* The plan and descriptor launches of an armed group, behind its classify (and
 * steer) launches on the slot's stream: over the records and descriptors where
 * the classify launch wrote and read them (s->h_qdesc), into the caller's
 * pinned arrays (in_place: mosrx__fwd_group_outputs filled the tables) or the
 * slot's buffers, which are then copied back per batch -- all n entries of each
 * array: those at and past the sent count then hold nothing of meaning. */
int mosrx__fwd_group_launch(mosrx_ctx *c, struct slot *s, const mosrx_batch *b, uint32_t nb, size_t rsz, int in_place,
                            const mosrx_slot_fwd_out *o);
/* The same with the firewall launch armed as well (mosrx_slot_acl): the plan
 * launch, mosrx__acl_group_launch over the group's plan arrays, then the
 * descriptor build's three -- never the one launch. */
int mosrx__fwd_group_launch_acl(mosrx_ctx *c, struct slot *s, const mosrx_batch *b, uint32_t nb, size_t rsz, int in_place,
                                const mosrx_slot_fwd_out *o, uint16_t *const *h_hit, uint32_t *h_counts);
/* A queue's forwarding conditions at run time (mosrx_queue_run asks before it
 * enqueues anything): -ENOENT with no tables installed, -EINVAL when rings are
 * attached and are fewer than the tables' netdevs. */
int mosrx__fwd_queue_check(const mosrx_ctx *c, const mosrx_queue *q);
/* The attached form's launches behind whatever the run already put on the
 * stream: the plan alone, the plan and the byte-ring build's three, or the
 * descriptor form's four -- or its one (mosrx_set_fwd_one). */
int mosrx__fwd_queue_launch(mosrx_ctx *c, const mosrx_queue *q, void *stream);
/* mosrx_time_op's block of TX outputs and scratch for the forwarding op `op`
 * over these batches (MOSRX_OP_FWD_PLAN needs none), kept by the context and
 * only grown; -ENOENT for a ring op with no tables installed. */
int mosrx__fwd_tmp_reserve(mosrx_ctx *c, int op, const mosrx_batch *b, uint32_t nb);
/* One enqueue of a forwarding op on batch b for mosrx_time_op: the plan from
 * the records in `out` (arg: rec_bytes | in_ifidx << 8) into `aux`, then the
 * op's build into stream s's part of that block. */
int mosrx__fwd_op(mosrx_ctx *c, int op, int arg, const mosrx_batch *b, void *out, void *aux, hipStream_t s);
/* The same flows with a queue that has firewall rules attached (q->acl): the
 * plan launch alone, and the attached build's launches alone (the three of
 * either ring form; nothing for a plan-only attachment) -- the firewall launch
 * goes between them, and the one-launch form is not taken. */
int mosrx__fwd_queue_launch_plan(mosrx_ctx *c, const mosrx_queue *q, void *stream);
int mosrx__fwd_queue_launch_build(mosrx_ctx *c, const mosrx_queue *q, void *stream);

/* ---- the firewall rules' host side (acl_api.c), as mosrx_api.c's flows reach it ---- */

/* A queue's condition at run time (mosrx_queue_run asks before it enqueues
 * anything): -ENOENT with no rules installed. */
int mosrx__acl_queue_check(const mosrx_ctx *c, const mosrx_queue *q);
/* The one launch over the queue's batches behind whatever the run already put
 * on the stream; with_plan: the forwarding attachment's plan arrays are amended. */
int mosrx__acl_queue_launch(mosrx_ctx *c, const mosrx_queue *q, int with_plan, void *stream);
/* An armed group at the submit: -ENOENT with no rules installed; batch i's hit
 * array (n its frame count): -EINVAL when NULL or odd and n != 0. */
int mosrx__acl_group_check(const mosrx_ctx *c);
int mosrx__acl_group_check_batch(uint16_t *const *h_hit, uint32_t i, uint32_t n);
/* The device addresses of an armed group's hit arrays into the slot's table,
 * when every one is pinned: 1, the launch may write in place; 0: copied back. */
int mosrx__acl_group_outputs(int device, struct slot *s, const mosrx_batch *b, uint32_t nb, uint16_t *const *h_hit);
/* The launch of an armed group on the slot's stream, over the records and
 * descriptors where the classify launch wrote and read them (s->h_qdesc);
 * with_plan: the plan arrays of the slot's forwarding table (s->d_fdesc, filled
 * by the plan launch ahead of it) are amended.  in_place: mosrx__acl_group_outputs
 * filled the table; else the slot's hits are copied back per batch. */
int mosrx__acl_group_launch(mosrx_ctx *c, struct slot *s, const mosrx_batch *b, uint32_t nb, size_t rsz, int in_place,
                            int with_plan, uint16_t *const *h_hit, uint32_t *h_counts);
/* The context's device copies, at close. */
void mosrx__acl_free(mosrx_ctx *c);

/* ---- NAT's host side (nat_api.c), as mosrx_api.c's flows reach it ---- */

/* A launch that reads the installed forwarding tables is about to go to stream
 * (fwd_api.c: plan-nat reads them as the plan launch does). */
void mosrx__fwd_mark_used(mosrx_ctx *c);
/* A queue's conditions at run time (mosrx_queue_run asks before it enqueues
 * anything): -EINVAL with no forwarding or with firewall rules attached, or under
 * skip_tcp_csum; -ENOENT with no bindings set. */
int mosrx__nat_queue_check(const mosrx_ctx *c, const mosrx_queue *q);
/* plan-nat over the queue's batches in the plan launch's place, and the patch
 * behind the byte-ring build; one launch each. */
int mosrx__nat_queue_launch_plan(mosrx_ctx *c, const mosrx_queue *q, void *stream);
int mosrx__nat_queue_launch_patch(mosrx_ctx *c, const mosrx_queue *q, void *stream);
/* The context's device copies, at close. */
void mosrx__nat_free(mosrx_ctx *c);

#endif
