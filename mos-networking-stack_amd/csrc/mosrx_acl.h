/*
 * mosrx_acl.h — shared between the C host library (acl_api.c) and the firewall
 * kernel (mosrx_acl.hip).  Plain C layout.
 */
#ifndef MOSRX_ACL_H
#define MOSRX_ACL_H

#include "mosrx_fwd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One lane per frame; the tile is the forwarding launches', so a queue's
 * tile_base[] (mosrx_fdesc) serves this launch too. */
#define MOSRX_ACL_THREADS 256u
#define MOSRX_ACL_TILE    MOSRX_FWD_TILE

/* The rules as the kernel reads them: one device block per mosrx_acl_set.
 * Structure of arrays, six dwords a rule, so a workgroup's copy into LDS reads
 * consecutive addresses.  The two wildcards are folded into the masks on the
 * host, so a rule is three tests of the form (key & mask) == value:
 *   an address of 0 (MatchAddr's '*') is stored with mask 0 and value 0, any
 *   other with the caller's mask and address as given;
 *   ports = sport | dport << 16 as the frame's dword at 14 + 4 * ihl holds them,
 *   port_mask 0xFFFF per side that is not 0 (MatchPort's '*'). */
typedef struct mosrx_acl_dev {
	uint32_t n, pad[3];
	uint32_t src_ip[MOSRX_ACL_MAX_RULES], src_mask[MOSRX_ACL_MAX_RULES];
	uint32_t dst_ip[MOSRX_ACL_MAX_RULES], dst_mask[MOSRX_ACL_MAX_RULES];
	uint32_t ports[MOSRX_ACL_MAX_RULES], port_mask[MOSRX_ACL_MAX_RULES];
	uint8_t  action[MOSRX_ACL_MAX_RULES];   /* read once per matched frame, from memory */
} mosrx_acl_dev;

/* A batch of the queue form (mosrx_queue_set_acl).  The plan array is not here:
 * it is the forwarding attachment's, read from the queue's mosrx_fdesc table,
 * whose tile_base[] is this table's.  An empty batch occupies no tile and its
 * pointers may be NULL. */
typedef struct mosrx_adesc {
	const uint8_t  *frames;
	const uint32_t *off;
	const uint16_t *len;
	const uint8_t  *rec;         /* n records of the launch's rec_bytes */
	uint16_t       *hit;
	uint32_t frames_bytes, n;
	uint32_t tile_base;
	uint32_t pad;
} mosrx_adesc;

typedef struct mosrx_aparams {
	/* the single batch (adesc NULL) */
	const uint8_t  *frames;
	const uint32_t *off;
	const uint16_t *len;
	const uint8_t  *rec;         /* n records of rec_bytes, aligned to rec_bytes */
	mosrx_fwd      *plan;        /* n, 8-byte aligned, or NULL */
	uint16_t       *hit;         /* n, 2-byte aligned */
	/* the queue form: nb batches, device-resident; fdesc the forwarding table
	 * parallel to it (its plan arrays), or NULL */
	const mosrx_adesc *adesc;
	const mosrx_fdesc *fdesc;
	const mosrx_acl_dev *tab;
	uint32_t *counts;            /* MOSRX_ACL_MAX_RULES, or NULL */
	uint32_t frames_bytes, n;
	uint32_t nb, total_tiles;    /* queue form */
	uint32_t rec_bytes;          /* 8 or 16 */
	int32_t  forward;            /* != 0: DROP rules amend the plan */
	uint32_t num_msp, listener;  /* the TCP arm of mosrx_mos_forwards */
} mosrx_aparams;

#ifdef __cplusplus
static_assert(sizeof(mosrx_adesc) == 56 && sizeof(mosrx_aparams) == 112, "firewall launch: 56-byte descriptor, 112-byte parameters");
#else
_Static_assert(sizeof(mosrx_adesc) == 56 && sizeof(mosrx_aparams) == 112, "firewall launch: 56-byte descriptor, 112-byte parameters");
#endif

/* The one launch on `stream`; 0, -EINVAL or -EIO.  Allocates nothing.  Nothing
 * to do (n == 0, or a queue of empty batches) launches nothing. */
int mosrx_launch_acl(const mosrx_aparams *ap, void *stream);

#ifdef __cplusplus
}
#endif
#endif
