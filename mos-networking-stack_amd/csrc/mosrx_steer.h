/*
 * mosrx_steer.h — shared between the C host library (mosrx_api.c) and the
 * queue-steering kernels (mosrx_steer.hip).  Plain C layout.  Kept out of
 * mosrx_internal.h, which is embedded for hipRTC: the fused kernels' source
 * does not change with it.
 */
#ifndef MOSRX_STEER_H
#define MOSRX_STEER_H

#include "../../include/mosrx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames per workgroup of the histogram and scatter launches: 8 waves, each
 * taking 4 slices of 64 frames in index order.  One histogram row (256 u32)
 * per tile: 0.5 B of scratch per frame. */
#define MOSRX_STEER_TILE    2048u
#define MOSRX_STEER_BINS    256u
#define MOSRX_STEER_THREADS 512u

/* One batch to steer (device resident for the multi-batch form), 32 bytes. */
typedef struct mosrx_sdesc {
	const uint8_t *rec;       /* n records of rec_bytes each, 4-byte aligned */
	uint32_t      *idx;       /* n */
	uint32_t      *qstart;    /* MOSRX_STEER_QSLOTS; NULL only with n == 0: nothing written */
	uint32_t       n;
	uint32_t       tile_base; /* the batch's first histogram row = its first workgroup in the launch */
} mosrx_sdesc;

/* The queue-major gather of one batch, parallel to its mosrx_sdesc (which
 * stays 32 bytes): the scatter pass also stores, in the order of idx,
 *   qrec[j] = rec[idx[j]]   whole records, rec and qrec aligned to rec_bytes
 *   qoff[j] = off[idx[j]], qlen[j] = len[idx[j]]   both given or both NULL
 * so queue q's share is three contiguous runs from qstart[q].  40 bytes. */
typedef struct mosrx_gdesc {
	const uint32_t *off;      /* the batch's descriptors; read only with qoff / qlen */
	const uint16_t *len;
	uint8_t        *qrec;     /* n records of rec_bytes */
	uint32_t       *qoff;     /* n, or NULL: records only */
	uint16_t       *qlen;     /* n, or NULL with qoff */
} mosrx_gdesc;

/* The side arrays of one batch, parallel to its mosrx_sdesc and mosrx_gdesc:
 * the gather form's side form also stores, in the order of idx,
 *   qfhash[j] = fhash[idx[j]], qmatch[j] = match[idx[j]]   u32
 *   qtcpinfo[j] = tcpinfo[idx[j]]                            12 bytes, whole
 * each pair on its own: a NULL destination is not gathered (nothing read,
 * nothing written).  All pointers 4-byte aligned.  48 bytes. */
typedef struct mosrx_xdesc {
	const uint32_t      *fhash;
	uint32_t            *qfhash;    /* n, or NULL */
	const uint32_t      *match;
	uint32_t            *qmatch;    /* n, or NULL */
	const mosrx_tcpinfo *tcpinfo;
	mosrx_tcpinfo       *qtcpinfo;  /* n, or NULL */
} mosrx_xdesc;

typedef struct mosrx_sparams {
	const mosrx_sdesc *desc;  /* nb entries in device-visible memory, or NULL: the one batch in `one` */
	mosrx_sdesc        one;
	uint32_t          *hist;  /* total_tiles rows of MOSRX_STEER_BINS u32 */
	uint32_t           nb;
	uint32_t           rec_bytes;   /* 8 or 16 */
	uint32_t           total_tiles;
	uint32_t           gather;      /* 1: the scatter pass is the gather form, over gdesc[] (with desc) or gone */
	const mosrx_gdesc *gdesc; /* nb entries parallel to desc[], or NULL */
	mosrx_gdesc        gone;  /* the gather of `one` */
	const mosrx_xdesc *xdesc; /* nb entries parallel to desc[] / gdesc[], or NULL */
	mosrx_xdesc        xone;  /* the side arrays of `one` */
	uint32_t           side;  /* 1 (with gather): the gather pass is its side form, over xdesc[] or xone */
	uint32_t           fused; /* 1: one launch, one workgroup per batch (every n <= MOSRX_STEER_ONE_MAX);
	                           * hist and tile_base unused, hist may be NULL */
} mosrx_sparams;

/* The three launches (histogram, scan, scatter) on `stream` (a hipStream_t);
 * 0, -EINVAL or -EIO.  Allocates nothing.  gather == 0 is the plain scatter
 * whatever gdesc / gone hold; with gather the single-batch form's pointers are
 * checked here (-EINVAL), a table's by whoever filled it.  side without gather
 * is -EINVAL; side == 0 is the gather form whatever xdesc / xone hold.
 * With `fused` the one launch of mosrx_steer_one_kernel instead, in the form
 * gather / side select: the same outputs, the same checks; the single-batch
 * form's n above MOSRX_STEER_ONE_MAX is -EINVAL. */
int mosrx_launch_steer(const mosrx_sparams *sp, void *stream);

#ifdef __cplusplus
}
#endif
#endif
