/*
 * mosrx_fwd.h — shared between the C host library (fwd_api.c) and the
 * forwarding kernels (mosrx_fwd.hip).  Plain C layout.  Kept out of
 * mosrx_internal.h, which is embedded for hipRTC: the fused kernels' source
 * does not change with it.
 */
#ifndef MOSRX_FWD_H
#define MOSRX_FWD_H

#include "../../include/mosrx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames per workgroup of the build's totals and copy launches: one lane per
 * frame for the scan inside the tile, then the tile's 16-byte TX units dealt
 * round robin over the same lanes.  One 16-byte row of scratch per tile. */
#define MOSRX_FWD_TILE    256u
#define MOSRX_FWD_THREADS 256u
#define MOSRX_FWD_ROW     16u   /* scratch bytes per tile */

/* The tables as the kernels read them: one device block per mosrx_fwd_set.
 * Structure of arrays, so a wave's walk reads one address per step (an LDS
 * broadcast once the plan kernel has copied the walked part in).  An ARP entry
 * with prefix 1 (GetDestinationHWaddr's exact-address form, arp.c:102-106) is
 * stored with mask ~0 and masked_ip = ip: one test serves both forms. */
typedef struct mosrx_fwd_dev {
	uint32_t num_routes, num_arp, num_netdevs;
	int32_t  has_nic_fwd;
	int8_t   nic_fwd[MOSRX_FWD_MAX_NETDEVS];
	uint8_t  netdev_haddr[MOSRX_FWD_MAX_NETDEVS][8];   /* 6 used */
	uint32_t r_mask[MOSRX_FWD_MAX_ROUTES], r_masked[MOSRX_FWD_MAX_ROUTES];
	int32_t  r_prefix[MOSRX_FWD_MAX_ROUTES], r_nif[MOSRX_FWD_MAX_ROUTES];
	uint32_t a_mask[MOSRX_FWD_MAX_ARP], a_masked[MOSRX_FWD_MAX_ARP];
	int32_t  a_prefix[MOSRX_FWD_MAX_ARP];
	uint8_t  a_haddr[MOSRX_FWD_MAX_ARP][8];            /* 6 used; read by the copy launch only */
} mosrx_fwd_dev;

typedef struct mosrx_fparams {
	/* the batch and its records */
	const uint8_t  *frames;
	const uint32_t *off;
	const uint16_t *len;
	const uint8_t  *rec;         /* n records of rec_bytes, aligned to rec_bytes (plan only) */
	const mosrx_fwd_dev *tab;
	mosrx_fwd      *plan;        /* n, 8-byte aligned: written by the plan, read by the build */
	uint32_t frames_bytes, n, rec_bytes;
	int32_t  in_ifidx;           /* 0 .. MOSRX_FWD_MAX_NETDEVS - 1 */
	int32_t  forward;            /* mosrx_mos_forwards' parameters */
	uint32_t num_msp, listener;
	/* the build's outputs */
	uint32_t  cap_units;         /* tx_cap / 16 */
	uint8_t  *tx;                /* 16-byte aligned */
	uint32_t *tx_off;
	uint16_t *tx_len;
	int8_t   *tx_nif;
	uint32_t *tx_src;
	uint32_t *tx_count;          /* 2 */
	uint32_t *scratch;           /* tiles rows of MOSRX_FWD_ROW bytes */
	uint32_t  tiles;
} mosrx_fparams;

/* The plan launch, and the build's three (totals, scan, copy), on `stream` (a
 * hipStream_t); 0, -EINVAL or -EIO.  Allocate nothing.  n == 0: the plan
 * launches nothing, the build its scan alone (tx_count = {0, 0}). */
int mosrx_launch_fwd_plan(const mosrx_fparams *fp, void *stream);
int mosrx_launch_fwd_build(const mosrx_fparams *fp, void *stream);

/* The ring form of the build (mosrx_fwd_build_rings_dev): its own parameters,
 * so the launches above are passed what they always were.  Scratch is one row
 * per tile of nrings entries of MOSRX_FWD_ROW bytes: {units, sent, 0, 0} after
 * the totals launch, {unit base lo, hi, entry base, 0} after the scan. */
typedef struct mosrx_rparams {
	const uint8_t  *frames;
	const uint32_t *off;
	const mosrx_fwd_dev *tab;
	const mosrx_fwd *plan;       /* n, 8-byte aligned */
	uint32_t frames_bytes, n;
	uint32_t nrings;             /* 1 .. MOSRX_FWD_MAX_NETDEVS */
	uint32_t cap_units;          /* ring_cap / 16; nrings * cap_units <= 2^28 */
	uint32_t tiles;
	uint8_t  *tx;                /* 16-byte aligned: nrings rings of cap_units units */
	uint32_t *tx_off;
	uint16_t *tx_len;
	uint32_t *tx_src;
	mosrx_fwd_ring *rings;       /* nrings, 16-byte aligned */
	uint32_t *scratch;           /* max(tiles, 1) * nrings rows */
} mosrx_rparams;

/* Its three launches (totals, scan, copy) on `stream`; 0, -EINVAL or -EIO.
 * n == 0: the scan alone (rings[q] = {0, 0, 0, 0}). */
int mosrx_launch_fwd_rings(const mosrx_rparams *rp, void *stream);

/* The batch-queue form (mosrx_queue_set_fwd): one device-resident descriptor
 * per batch of the queue.  Tiles of MOSRX_FWD_TILE frames never straddle
 * batches, so one tile_base[] serves the plan, totals and copy launches (grid =
 * total_tiles, a workgroup finding its batch by binary search of tile_base[]
 * as the steer queue form does), and a batch's scratch rows start at
 * tile_base * nrings.  An empty batch occupies no tile (its tile_base is its
 * successor's) and its pointers other than rings may be NULL. */
typedef struct mosrx_fdesc {
	const uint8_t  *frames;
	const uint32_t *off;
	const uint16_t *len;
	const uint8_t  *rec;         /* n records of the launch's rec_bytes */
	mosrx_fwd      *plan;        /* n, 8-byte aligned */
	uint8_t        *tx;          /* the five TX outputs of mosrx_rparams; unused by a plan-only launch */
	uint32_t       *tx_off;
	uint16_t       *tx_len;
	uint32_t       *tx_src;
	mosrx_fwd_ring *rings;
	uint32_t frames_bytes, n;
	uint32_t in_ifidx;           /* 0 .. MOSRX_FWD_MAX_NETDEVS - 1 */
	uint32_t tile_base;          /* the batch's first tile = its first workgroup in the tiled launches */
} mosrx_fdesc;

typedef struct mosrx_fqparams {
	const mosrx_fdesc   *desc;   /* nb, device-resident */
	const mosrx_fwd_dev *tab;
	uint32_t *scratch;           /* max(total_tiles, 1) * nrings rows of MOSRX_FWD_ROW bytes; plan only: unused */
	uint32_t nb, total_tiles;
	uint32_t rec_bytes;          /* 8 or 16 */
	int32_t  forward;            /* mosrx_mos_forwards' parameters */
	uint32_t num_msp, listener;
	uint32_t nrings;             /* 1 .. MOSRX_FWD_MAX_NETDEVS */
	uint32_t cap_units;          /* ring_cap / 16; nrings * cap_units <= 2^28 */
} mosrx_fqparams;

#ifdef __cplusplus
static_assert(sizeof(mosrx_fdesc) == 96 && sizeof(mosrx_fqparams) == 56, "queue form: 96-byte descriptor, 56-byte parameters");
#else
_Static_assert(sizeof(mosrx_fdesc) == 96 && sizeof(mosrx_fqparams) == 56, "queue form: 96-byte descriptor, 56-byte parameters");
#endif

/* The plan launch over every batch of the queue and, with_build, the ring
 * build's three (totals, scan with one workgroup per batch, copy) on `stream`:
 * four launches whatever nb is; 0, -EINVAL or -EIO.  Allocates nothing.  A
 * queue of empty batches launches the scan alone (every rings[q] = {0,0,0,0}). */
int mosrx_launch_fwd_queue(const mosrx_fqparams *fq, int with_build, void *stream);

/* The descriptor form of the ring build (mosrx_fwd_desc_rings_dev): per sent
 * frame its source index, TX length and 12 rewritten address bytes in place of
 * the frame.  Scratch as the ring form's. */
typedef struct mosrx_dparams {
	const uint8_t  *frames;
	const uint32_t *off;
	const mosrx_fwd_dev *tab;
	const mosrx_fwd *plan;       /* n, 8-byte aligned */
	uint32_t frames_bytes, n;
	uint32_t nrings;             /* 1 .. MOSRX_FWD_MAX_NETDEVS */
	uint32_t tiles;
	uint32_t *tx_src;
	uint16_t *tx_len;
	uint32_t *tx_mac;            /* three dwords per entry */
	mosrx_fwd_ring *rings;       /* nrings, 16-byte aligned */
	uint32_t *scratch;           /* max(tiles, 1) * nrings rows */
} mosrx_dparams;

/* Its three launches (the ring form's totals and scan, then the store) on
 * `stream`; 0, -EINVAL or -EIO.  n == 0: the scan alone. */
int mosrx_launch_fwd_desc(const mosrx_dparams *dp, void *stream);

/* Its batch-queue form (mosrx_queue_set_fwd_desc): the plan, totals and scan
 * launches read the queue's mosrx_fdesc table (tx and tx_off unused), the store
 * launch this one, built over the same tile_base[]. */
typedef struct mosrx_ddesc {
	const uint8_t  *frames;
	const uint32_t *off;
	const mosrx_fwd *plan;
	uint32_t       *tx_src;
	uint16_t       *tx_len;
	uint32_t       *tx_mac;
	mosrx_fwd_ring *rings;
	uint32_t frames_bytes, n;
	uint32_t tile_base;
	uint32_t pad;
} mosrx_ddesc;

typedef struct mosrx_dqparams {
	const mosrx_ddesc   *desc;   /* nb, device-resident */
	const mosrx_fwd_dev *tab;
	uint32_t *scratch;           /* the fqparams' */
	uint32_t nb, total_tiles;
	uint32_t nrings;
	uint32_t pad;
} mosrx_dqparams;

#ifdef __cplusplus
static_assert(sizeof(mosrx_ddesc) == 72 && sizeof(mosrx_dqparams) == 40, "descriptor queue form: 72-byte descriptor, 40-byte parameters");
#else
_Static_assert(sizeof(mosrx_ddesc) == 72 && sizeof(mosrx_dqparams) == 40, "descriptor queue form: 72-byte descriptor, 40-byte parameters");
#endif

/* Plan, totals, scan (one workgroup per batch) and store over every batch of
 * the queue: four launches whatever nb is; 0, -EINVAL or -EIO.  fq->cap_units
 * is not looked at.  A queue of empty batches launches the scan alone. */
int mosrx_launch_fwd_desc_queue(const mosrx_fqparams *fq, const mosrx_dqparams *dq, void *stream);

/* The build launches of the two queue forms without the plan launch ahead of
 * them (three each: totals, scan, copy / store), for a run that puts a launch
 * of its own between the plan and the build (the firewall rules,
 * mosrx_queue_set_acl); the plan alone is mosrx_launch_fwd_queue(fq, 0).  The
 * same kernels with the same parameters, and the same refusals. */
int mosrx_launch_fwd_queue_build(const mosrx_fqparams *fq, void *stream);
int mosrx_launch_fwd_desc_queue_build(const mosrx_fqparams *fq, const mosrx_dqparams *dq, void *stream);

/* The one-launch form (mosrx_set_fwd_one): the plan and the descriptor rings of
 * every batch by one workgroup per batch, the same bytes as the four launches
 * above (no scratch is read or written).  The batches are the queue form's two
 * tables as they are (tile_base is not looked at), or, with ddesc NULL, the one
 * batch in onef / oned (nb = 1).  rec_bytes 0: no plan -- the records are read
 * from ddesc[].plan, fdesc and onef are not looked at, and the launch is
 * mosrx_launch_fwd_desc's three.  Every batch has n <= MOSRX_FWD_ONE_MAX: the
 * caller's to see to for a table (a workgroup stops after that many frames). */
typedef struct mosrx_oparams {
	const mosrx_fdesc   *fdesc;  /* nb, device-resident: frames' len, rec, in_ifidx and the plan to write */
	const mosrx_ddesc   *ddesc;  /* nb, device-resident; NULL: onef / oned */
	const mosrx_fwd_dev *tab;
	uint32_t nb;
	uint32_t rec_bytes;          /* 8 or 16: plan first; 0: the plan is there */
	int32_t  forward;            /* mosrx_mos_forwards' parameters */
	uint32_t num_msp, listener;
	uint32_t nrings;             /* 1 .. MOSRX_FWD_MAX_NETDEVS */
	mosrx_fdesc onef;
	mosrx_ddesc oned;
} mosrx_oparams;

#ifdef __cplusplus
static_assert(sizeof(mosrx_oparams) == 216, "one-launch form: 216-byte parameters");
#else
_Static_assert(sizeof(mosrx_oparams) == 216, "one-launch form: 216-byte parameters");
#endif

/* One launch of nb workgroups on `stream`; 0, -EINVAL or -EIO.  Allocates
 * nothing.  An empty batch's workgroup writes its zeroed rings and nothing else. */
int mosrx_launch_fwd_one(const mosrx_oparams *op, void *stream);

#ifdef __cplusplus
}
#endif
#endif
