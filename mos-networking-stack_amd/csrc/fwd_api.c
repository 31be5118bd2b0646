/*
 * fwd_api.c — host side of forwarding (include/mosrx.h; kernels in mosrx_fwd.hip).
 *
 * Every forwarding entry point, its argument refusals and its launches.
 * mosrx_api.c keeps the flows forwarding hangs on (the group submit, the queue
 * run, the timing ops, the slots' and queues' allocation and release) and
 * reaches this file through the mosrx__fwd_* functions of mosrx_ctx.h.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "mosrx_ctx.h"

/* ---- sizes --------------------------------------------------------------------- */

static uint32_t fwd_tiles(uint32_t n)
{
	return (uint32_t)(((size_t)n + MOSRX_FWD_TILE - 1) / MOSRX_FWD_TILE);
}

size_t mosrx_fwd_scratch_bytes(uint32_t n)
{
	const size_t tiles = fwd_tiles(n);
	return (tiles ? tiles : 1) * MOSRX_FWD_ROW;
}

uint32_t mosrx_fwd_tile(void) { return MOSRX_FWD_TILE; }

/* one row per tile and ring; nrings outside 1 .. MOSRX_FWD_MAX_NETDEVS is
 * clamped, so the size is defined (and monotone) for every argument */
size_t mosrx_fwd_rings_scratch_bytes(uint32_t n, uint32_t nrings)
{
	const size_t tiles = fwd_tiles(n);
	const size_t q = nrings < 1 ? 1 : nrings > MOSRX_FWD_MAX_NETDEVS ? MOSRX_FWD_MAX_NETDEVS : nrings;
	return (tiles ? tiles : 1) * q * MOSRX_FWD_ROW;
}

size_t mosrx_fwd_desc_scratch_bytes(uint32_t n, uint32_t nrings)
{
	return mosrx_fwd_rings_scratch_bytes(n, nrings);
}

/* ---- the context's settings and tables ------------------------------------------ */

int mosrx_fwd_set_listener(mosrx_ctx *c, int listener)
{
	if (!c)
		return -EINVAL;
	c->fwd_listener = listener != 0;
	return 0;
}

int mosrx_set_fwd_one(mosrx_ctx *c, uint32_t max_frames)
{
	if (!c || max_frames > MOSRX_FWD_ONE_MAX)
		return -EINVAL;
	c->fwd_one = max_frames;
	return 0;
}

uint32_t mosrx_get_fwd_one(const mosrx_ctx *c) { return c ? c->fwd_one : 0; }

uint64_t mosrx_fwd_one_count(const mosrx_ctx *c) { return c ? c->fwd_one_count : 0; }

/* The tables go to the next buffer of a pool, as the BPF instruction buffers
 * do (bpf_api.c stage_insns): launches submitted earlier may still read the
 * copy they were given, so a buffer is written again only after those launches
 * drained, and only if a launch may have read it since its last write. */
int mosrx_fwd_set(mosrx_ctx *c, const mosrx_fwd_tables *t)
{
	mosrx_fwd_dev *h;
	uint32_t i, k;
	int rc;
	if (!c)
		return -EINVAL;
	if (!t) {
		c->d_fwd = NULL;
		c->fwd_num_netdevs = 0;
		return 0;
	}
	if (t->num_routes > MOSRX_FWD_MAX_ROUTES || t->num_arp > MOSRX_FWD_MAX_ARP ||
	    t->num_netdevs > MOSRX_FWD_MAX_NETDEVS)
		return -EINVAL;
	for (i = 0; i < t->num_routes; i++)
		if (t->routes[i].nif < 0 || (uint32_t)t->routes[i].nif >= t->num_netdevs)
			return -EINVAL;
	for (i = 0; t->has_nic_fwd && i < MOSRX_FWD_MAX_NETDEVS; i++)
		if (t->nic_fwd[i] != -1 && (t->nic_fwd[i] < 0 || (uint32_t)t->nic_fwd[i] >= t->num_netdevs))
			return -EINVAL;
	if (!(h = calloc(1, sizeof(*h))))
		return -ENOMEM;
	h->num_routes = t->num_routes;
	h->num_arp = t->num_arp;
	h->num_netdevs = t->num_netdevs;
	h->has_nic_fwd = t->has_nic_fwd != 0;
	memcpy(h->nic_fwd, t->nic_fwd, sizeof(h->nic_fwd));
	for (i = 0; i < MOSRX_FWD_MAX_NETDEVS; i++)
		memcpy(h->netdev_haddr[i], t->netdev_haddr[i], 6);
	for (i = 0; i < t->num_routes; i++) {
		h->r_mask[i] = t->routes[i].mask;
		h->r_masked[i] = t->routes[i].masked_ip;
		h->r_prefix[i] = t->routes[i].prefix;
		h->r_nif[i] = t->routes[i].nif;
	}
	for (i = 0; i < t->num_arp; i++) {
		/* prefix 1 is GetDestinationHWaddr's exact-address form (arp.c:102-106) */
		const int exact = t->arp[i].prefix == 1;
		h->a_mask[i] = exact ? 0xFFFFFFFFu : t->arp[i].mask;
		h->a_masked[i] = exact ? t->arp[i].ip : t->arp[i].masked_ip;
		h->a_prefix[i] = t->arp[i].prefix;
		memcpy(h->a_haddr[i], t->arp[i].haddr, 6);
	}
	rc = 0;
	k = c->fwd_pool_next;
	if (hipSetDevice(c->device) != hipSuccess)
		rc = -EIO;
	if (!rc && !c->d_fwd_pool[k] && hipMalloc((void **)&c->d_fwd_pool[k], sizeof(*h)) != hipSuccess)
		rc = -ENOMEM;
	if (!rc && c->fwd_pool_used[k] && !(rc = mosrx__drain(c)))
		memset(c->fwd_pool_used, 0, sizeof(c->fwd_pool_used));
	if (!rc && hipMemcpy(c->d_fwd_pool[k], h, sizeof(*h), hipMemcpyHostToDevice) != hipSuccess)
		rc = -EIO;
	free(h);
	if (rc)
		return rc;
	c->d_fwd = c->d_fwd_pool[k];
	c->fwd_num_netdevs = t->num_netdevs;
	c->fwd_pool_next = (k + 1) % MOSRX_FWD_POOL;
	return 0;
}

/* A launch that reads the installed tables is about to go to stream. */
static void fwd_mark_used(mosrx_ctx *c)
{
	c->fwd_pool_used[(c->fwd_pool_next + MOSRX_FWD_POOL - 1) % MOSRX_FWD_POOL] = 1;
}

void mosrx__fwd_mark_used(mosrx_ctx *c) { fwd_mark_used(c); }

/* What a planning launch takes from the context: the installed tables and
 * mosrx_mos_forwards' parameters, into the fields of mosrx_fparams,
 * mosrx_fqparams or mosrx_oparams that carry them. */
static void fwd_ctx_params(const mosrx_ctx *c, const mosrx_fwd_dev **tab, int32_t *forward, uint32_t *num_msp,
                           uint32_t *listener)
{
	*tab = c->d_fwd;
	*forward = c->params.forward;
	*num_msp = c->params.num_msp;
	*listener = c->fwd_listener;
}

/* ---- argument refusals ----------------------------------------------------------- */

/* non-NULL and aligned to a (a power of two) */
static int aligned(const void *p, uintptr_t a)
{
	return p && !((uintptr_t)p & (a - 1));
}

static int nrings_ok(uint32_t nrings)
{
	return nrings >= 1 && nrings <= MOSRX_FWD_MAX_NETDEVS;
}

/* The plan's arguments for batch b: the record size, the input netdev, the plan
 * array, and -- of a batch with frames -- records aligned to their size. */
static int plan_args_ok(const mosrx_batch *b, const void *d_rec, int rec_bytes, int in_ifidx, const mosrx_fwd *d_plan)
{
	return aligned(d_plan, 8) && (rec_bytes == 8 || rec_bytes == 16) && in_ifidx >= 0 &&
	       in_ifidx < MOSRX_FWD_MAX_NETDEVS && (!b->n || aligned(d_rec, (uintptr_t)rec_bytes));
}

/* The descriptor outputs of one batch: its ring rows whatever it holds (aligned
 * to ra), its three arrays when `arrays` -- always for a *_dev call, for a
 * batch with frames in a queue or group. */
static int desc_out_ok(int arrays, const uint32_t *tx_src, const uint16_t *tx_len, const uint32_t *tx_mac,
                       const mosrx_fwd_ring *rings, uintptr_t ra)
{
	return aligned(rings, ra) && (!arrays || (aligned(tx_src, 4) && aligned(tx_len, 2) && aligned(tx_mac, 4)));
}

/* ... of a *_dev call on n frames, with its nrings and scratch */
static int desc_args_ok(uint32_t n, uint32_t nrings, const uint32_t *tx_src, const uint16_t *tx_len,
                        const uint32_t *tx_mac, const mosrx_fwd_ring *rings, const void *scratch, size_t scratch_bytes)
{
	return nrings_ok(nrings) && desc_out_ok(1, tx_src, tx_len, tx_mac, rings, 16) && aligned(scratch, 16) &&
	       scratch_bytes >= mosrx_fwd_desc_scratch_bytes(n, nrings);
}

/* The byte-ring outputs of one batch, by desc_out_ok's rule. */
static int ring_out_ok(int arrays, const uint8_t *tx, const uint32_t *tx_off, const uint16_t *tx_len,
                       const uint32_t *tx_src, const mosrx_fwd_ring *rings)
{
	return aligned(rings, 16) &&
	       (!arrays || (aligned(tx, 16) && aligned(tx_off, 4) && aligned(tx_len, 2) && aligned(tx_src, 4)));
}

/* nrings rings of ring_cap bytes each: whole 16-byte units, and together within
 * what tx_off, a u32, addresses */
static int ring_cap_ok(uint64_t ring_cap, uint32_t nrings)
{
	return nrings_ok(nrings) && !(ring_cap & 15) && ring_cap <= (1ull << 32) && ring_cap * nrings <= (1ull << 32);
}

/* The batch itself: mosrx__check_batch's code, -EINVAL for off[] / len[] not
 * aligned to their loads; then fp holds it, and the installed tables. */
static int fwd_batch(const mosrx_ctx *c, const mosrx_batch *b, mosrx_fparams *fp)
{
	int rc;
	if ((rc = mosrx__check_batch(b, 1)))
		return rc;
	if (b->n && ((((uintptr_t)b->off) & 3) || (((uintptr_t)b->len) & 1)))
		return -EINVAL;
	memset(fp, 0, sizeof(*fp));
	fp->frames = b->frames;
	fp->off = b->off;
	fp->len = b->len;
	fp->frames_bytes = (uint32_t)b->frames_bytes;
	fp->n = b->n;
	fp->tab = c->d_fwd;
	return 0;
}

/* ---- one device-resident batch --------------------------------------------------- */

int mosrx_fwd_plan_dev(mosrx_ctx *c, const mosrx_batch *b, const void *d_rec, int rec_bytes, int in_ifidx,
                       mosrx_fwd *d_plan, void *stream)
{
	mosrx_fparams fp;
	hipStream_t s;
	int rc;
	if (!c || !b || !plan_args_ok(b, d_rec, rec_bytes, in_ifidx, d_plan))
		return -EINVAL;
	if ((rc = fwd_batch(c, b, &fp)))
		return rc;
	if (!c->d_fwd)
		return -ENOENT;
	if (b->n == 0)
		return 0;
	fp.rec = (const uint8_t *)d_rec;
	fp.rec_bytes = (uint32_t)rec_bytes;
	fp.in_ifidx = in_ifidx;
	fp.plan = d_plan;
	fwd_ctx_params(c, &fp.tab, &fp.forward, &fp.num_msp, &fp.listener);
	s = stream ? (hipStream_t)stream : c->stream;
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	rc = mosrx_launch_fwd_plan(&fp, (void *)s);
	mosrx__note_stream(c, s);   /* (after the launch: its event covers it) */
	return rc;
}

int mosrx_fwd_build_dev(mosrx_ctx *c, const mosrx_batch *b, const mosrx_fwd *d_plan, uint8_t *d_tx_frames,
                        uint64_t tx_cap, uint32_t *d_tx_off, uint16_t *d_tx_len, int8_t *d_tx_nif,
                        uint32_t *d_tx_src, uint32_t *d_tx_count, void *d_scratch, size_t scratch_bytes, void *stream)
{
	mosrx_fparams fp;
	hipStream_t s;
	int rc;
	if (!c || !b || !aligned(d_plan, 8) || !aligned(d_tx_frames, 16) || !aligned(d_tx_off, 4) || !aligned(d_tx_len, 2) ||
	    !d_tx_nif || !aligned(d_tx_src, 4) || !aligned(d_tx_count, 4) || !aligned(d_scratch, 16) ||
	    scratch_bytes < mosrx_fwd_scratch_bytes(b->n))
		return -EINVAL;
	if ((rc = fwd_batch(c, b, &fp)))
		return rc;
	if (!c->d_fwd)
		return -ENOENT;
	fp.plan = (mosrx_fwd *)d_plan;
	/* tx_off is a u32: room past 4 GiB is never used */
	fp.cap_units = (uint32_t)((tx_cap > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : tx_cap) / 16);
	fp.tx = d_tx_frames;
	fp.tx_off = d_tx_off;
	fp.tx_len = d_tx_len;
	fp.tx_nif = d_tx_nif;
	fp.tx_src = d_tx_src;
	fp.tx_count = d_tx_count;
	fp.scratch = (uint32_t *)d_scratch;
	fp.tiles = fwd_tiles(b->n);
	s = stream ? (hipStream_t)stream : c->stream;
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	rc = mosrx_launch_fwd_build(&fp, (void *)s);
	mosrx__note_stream(c, s);
	return rc;
}

int mosrx_fwd_build_rings_dev(mosrx_ctx *c, const mosrx_batch *b, const mosrx_fwd *d_plan, uint8_t *d_tx_frames,
                              uint64_t ring_cap, uint32_t nrings, uint32_t *d_tx_off, uint16_t *d_tx_len,
                              uint32_t *d_tx_src, mosrx_fwd_ring *d_rings, void *d_scratch, size_t scratch_bytes,
                              void *stream)
{
	mosrx_fparams fp;
	mosrx_rparams rp;
	hipStream_t s;
	int rc;
	if (!c || !b || !aligned(d_plan, 8) || !ring_out_ok(1, d_tx_frames, d_tx_off, d_tx_len, d_tx_src, d_rings) ||
	    !ring_cap_ok(ring_cap, nrings) || !aligned(d_scratch, 16) ||
	    scratch_bytes < mosrx_fwd_rings_scratch_bytes(b->n, nrings))
		return -EINVAL;
	if ((rc = fwd_batch(c, b, &fp)))
		return rc;
	if (!c->d_fwd)
		return -ENOENT;
	if (nrings < c->fwd_num_netdevs)
		return -EINVAL;
	memset(&rp, 0, sizeof(rp));
	rp.frames = fp.frames;
	rp.off = fp.off;
	rp.tab = fp.tab;
	rp.plan = d_plan;
	rp.frames_bytes = fp.frames_bytes;
	rp.n = fp.n;
	rp.nrings = nrings;
	rp.cap_units = (uint32_t)(ring_cap / 16);
	rp.tiles = fwd_tiles(b->n);
	rp.tx = d_tx_frames;
	rp.tx_off = d_tx_off;
	rp.tx_len = d_tx_len;
	rp.tx_src = d_tx_src;
	rp.rings = d_rings;
	rp.scratch = (uint32_t *)d_scratch;
	s = stream ? (hipStream_t)stream : c->stream;
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	rc = mosrx_launch_fwd_rings(&rp, (void *)s);
	mosrx__note_stream(c, s);
	return rc;
}

/* ---- the descriptor form of the ring build ---- */

/* The descriptor launch's parameters over the checked batch in fp. */
static void dparams_fill(mosrx_dparams *dp, const mosrx_fparams *fp, const mosrx_fwd *d_plan, uint32_t nrings,
                         uint32_t *d_tx_src, uint16_t *d_tx_len, uint32_t *d_tx_mac, mosrx_fwd_ring *d_rings,
                         void *d_scratch)
{
	memset(dp, 0, sizeof(*dp));
	dp->frames = fp->frames;
	dp->off = fp->off;
	dp->tab = fp->tab;
	dp->plan = d_plan;
	dp->frames_bytes = fp->frames_bytes;
	dp->n = fp->n;
	dp->nrings = nrings;
	dp->tiles = fwd_tiles(fp->n);
	dp->tx_src = d_tx_src;
	dp->tx_len = d_tx_len;
	dp->tx_mac = d_tx_mac;
	dp->rings = d_rings;
	dp->scratch = (uint32_t *)d_scratch;
}

/* The one launch over the single batch in dp (n <= MOSRX_FWD_ONE_MAX); with fp,
 * the plan first, from its records, length array, in_ifidx and record size. */
static int fwd_one_batch(mosrx_ctx *c, const mosrx_dparams *dp, const mosrx_fparams *fp, hipStream_t s)
{
	mosrx_oparams op;
	int rc;
	memset(&op, 0, sizeof(op));
	op.tab = dp->tab;
	op.nb = 1;
	op.nrings = dp->nrings;
	op.oned.frames = dp->frames;
	op.oned.off = dp->off;
	op.oned.plan = dp->plan;
	op.oned.tx_src = dp->tx_src;
	op.oned.tx_len = dp->tx_len;
	op.oned.tx_mac = dp->tx_mac;
	op.oned.rings = dp->rings;
	op.oned.frames_bytes = dp->frames_bytes;
	op.oned.n = dp->n;
	if (fp) {
		fwd_ctx_params(c, &op.tab, &op.forward, &op.num_msp, &op.listener);
		op.rec_bytes = fp->rec_bytes;
		op.onef.len = fp->len;
		op.onef.rec = fp->rec;
		op.onef.plan = (mosrx_fwd *)dp->plan;
		op.onef.in_ifidx = (uint32_t)fp->in_ifidx;
	}
	if (!(rc = mosrx_launch_fwd_one(&op, (void *)s)))
		c->fwd_one_count++;
	return rc;
}

int mosrx_fwd_desc_rings_dev(mosrx_ctx *c, const mosrx_batch *b, const mosrx_fwd *d_plan, uint32_t nrings,
                             uint32_t *d_tx_src, uint16_t *d_tx_len, uint32_t *d_tx_mac, mosrx_fwd_ring *d_rings,
                             void *d_scratch, size_t scratch_bytes, void *stream)
{
	mosrx_fparams fp;
	mosrx_dparams dp;
	hipStream_t s;
	int rc;
	if (!c || !b || !aligned(d_plan, 8) ||
	    !desc_args_ok(b->n, nrings, d_tx_src, d_tx_len, d_tx_mac, d_rings, d_scratch, scratch_bytes))
		return -EINVAL;
	if ((rc = fwd_batch(c, b, &fp)))
		return rc;
	if (!c->d_fwd)
		return -ENOENT;
	if (nrings < c->fwd_num_netdevs)
		return -EINVAL;
	dparams_fill(&dp, &fp, d_plan, nrings, d_tx_src, d_tx_len, d_tx_mac, d_rings, d_scratch);
	s = stream ? (hipStream_t)stream : c->stream;
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	if (c->fwd_one && b->n <= c->fwd_one)
		rc = fwd_one_batch(c, &dp, NULL, s);   /* (the scratch is left as it is) */
	else
		rc = mosrx_launch_fwd_desc(&dp, (void *)s);
	mosrx__note_stream(c, s);
	return rc;
}

/* MOSRX_OP_FWD_DESC under mosrx_set_fwd_one's limit: mosrx_fwd_plan_dev and
 * mosrx_fwd_desc_rings_dev on one batch, their refusals in their order, as one
 * launch. */
static int fwd_plan_desc_one(mosrx_ctx *c, const mosrx_batch *b, const void *d_rec, int rec_bytes, int in_ifidx,
                             mosrx_fwd *d_plan, uint32_t nrings, uint32_t *d_tx_src, uint16_t *d_tx_len,
                             uint32_t *d_tx_mac, mosrx_fwd_ring *d_rings, void *d_scratch, size_t scratch_bytes,
                             hipStream_t s)
{
	mosrx_fparams fp;
	mosrx_dparams dp;
	int rc;
	if (!c || !b || !plan_args_ok(b, d_rec, rec_bytes, in_ifidx, d_plan))
		return -EINVAL;
	if ((rc = fwd_batch(c, b, &fp)))
		return rc;
	if (!c->d_fwd)
		return -ENOENT;
	if (!desc_args_ok(b->n, nrings, d_tx_src, d_tx_len, d_tx_mac, d_rings, d_scratch, scratch_bytes) ||
	    nrings < c->fwd_num_netdevs)
		return -EINVAL;
	if (!s)
		s = c->stream;
	fp.rec = (const uint8_t *)d_rec;
	fp.rec_bytes = (uint32_t)rec_bytes;
	fp.in_ifidx = in_ifidx;
	dparams_fill(&dp, &fp, d_plan, nrings, d_tx_src, d_tx_len, d_tx_mac, d_rings, d_scratch);
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	rc = fwd_one_batch(c, &dp, &fp, s);
	mosrx__note_stream(c, s);
	return rc;
}

/* ---- the batch tables of a queue or group ----------------------------------------- */

/* The forwarding descriptor of a batch from its classify descriptor d: the
 * records are where the classify launch writes them, the plan goes to `plan`,
 * the batch's first tile is tile_base.  An empty batch keeps no pointer but
 * rings; the build's four outputs are the caller's to add.  Returns the
 * batch's tile count. */
static uint32_t fdesc_fill(mosrx_fdesc *f, const mosrx_qdesc *d, uint32_t in_ifidx, uint32_t tile_base, mosrx_fwd *plan,
                           mosrx_fwd_ring *rings)
{
	memset(f, 0, sizeof(*f));
	f->rings = rings;
	f->n = d->n;
	f->in_ifidx = in_ifidx;
	f->tile_base = tile_base;
	if (d->n) {
		f->frames = d->frames;
		f->off = d->off;
		f->len = d->len;
		f->rec = (const uint8_t *)d->out;
		f->plan = plan;
		f->frames_bytes = d->frames_bytes;
	}
	return fwd_tiles(d->n);
}

/* The store launch's descriptor of the same batch, with its three arrays. */
static void ddesc_from(mosrx_ddesc *g, const mosrx_fdesc *f, uint32_t *tx_src, uint16_t *tx_len, uint32_t *tx_mac)
{
	g->frames = f->frames;
	g->off = f->off;
	g->plan = f->plan;
	g->tx_src = f->n ? tx_src : NULL;
	g->tx_len = f->n ? tx_len : NULL;
	g->tx_mac = f->n ? tx_mac : NULL;
	g->rings = f->rings;
	g->frames_bytes = f->frames_bytes;
	g->n = f->n;
	g->tile_base = f->tile_base;
	g->pad = 0;
}

/* The parameters of the plan (and byte-ring) launches over a table of nb batches. */
static void fqparams_fill(const mosrx_ctx *c, mosrx_fqparams *fq, const mosrx_fdesc *fdesc, uint32_t *scratch,
                          uint32_t nb, uint32_t tiles, uint32_t rec_bytes, uint32_t nrings)
{
	memset(fq, 0, sizeof(*fq));
	fwd_ctx_params(c, &fq->tab, &fq->forward, &fq->num_msp, &fq->listener);
	fq->desc = fdesc;
	fq->scratch = scratch;
	fq->nb = nb;
	fq->total_tiles = tiles;
	fq->rec_bytes = rec_bytes;
	fq->nrings = nrings;
}

/* The plan and descriptor launches over a queue's or a group's two tables (fq
 * over the first, ddesc the second), whose largest batch has maxn frames: the
 * one launch when the context's limit admits every batch (mosrx_set_fwd_one),
 * else -- and always with the limit at 0 -- the four. */
static int fwd_desc_queue_launch(mosrx_ctx *c, const mosrx_fqparams *fq, const mosrx_ddesc *ddesc, uint32_t maxn,
                                 void *stream)
{
	mosrx_oparams op;
	int rc;
	if (!c->fwd_one || maxn > c->fwd_one) {
		mosrx_dqparams dq;
		memset(&dq, 0, sizeof(dq));
		dq.desc = ddesc;
		dq.tab = fq->tab;
		dq.scratch = fq->scratch;
		dq.nb = fq->nb;
		dq.total_tiles = fq->total_tiles;
		dq.nrings = fq->nrings;
		return mosrx_launch_fwd_desc_queue(fq, &dq, stream);
	}
	memset(&op, 0, sizeof(op));
	op.fdesc = fq->desc;
	op.ddesc = ddesc;
	op.tab = fq->tab;
	op.nb = fq->nb;
	op.rec_bytes = fq->rec_bytes;
	op.forward = fq->forward;
	op.num_msp = fq->num_msp;
	op.listener = fq->listener;
	op.nrings = fq->nrings;
	if (!(rc = mosrx_launch_fwd_one(&op, stream)))
		c->fwd_one_count++;
	return rc;
}

/* ---- forwarding over a batch queue (mosrx_queue_set_fwd*) -------------------------- */

int mosrx__fwd_queue_check(const mosrx_ctx *c, const mosrx_queue *q)
{
	if (!c->d_fwd)
		return -ENOENT;
	if ((q->fwd_build || q->fwd_desc) && q->fwd_nrings < c->fwd_num_netdevs)
		return -EINVAL;
	return 0;
}

int mosrx__fwd_queue_launch(mosrx_ctx *c, const mosrx_queue *q, void *stream)
{
	mosrx_fqparams fq;
	const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	int rc;
	fqparams_fill(c, &fq, q->d_fdesc, q->d_fscratch, q->nb, q->fwd_tiles, q->compact ? 8u : 16u, q->fwd_nrings);
	fq.cap_units = q->fwd_cap_units;
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	if (q->fwd_desc)
		rc = fwd_desc_queue_launch(c, &fq, q->d_ddesc, q->fwd_maxn, (void *)s);
	else
		rc = mosrx_launch_fwd_queue(&fq, q->fwd_build, (void *)s);
	mosrx__note_stream(c, s);   /* (after the launches: its event covers them) */
	return rc;
}

int mosrx__fwd_queue_launch_plan(mosrx_ctx *c, const mosrx_queue *q, void *stream)
{
	mosrx_fqparams fq;
	const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	int rc;
	fqparams_fill(c, &fq, q->d_fdesc, q->d_fscratch, q->nb, q->fwd_tiles, q->compact ? 8u : 16u, q->fwd_nrings);
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	rc = mosrx_launch_fwd_queue(&fq, 0, (void *)s);
	mosrx__note_stream(c, s);
	return rc;
}

int mosrx__fwd_queue_launch_build(mosrx_ctx *c, const mosrx_queue *q, void *stream)
{
	mosrx_fqparams fq;
	const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	int rc;
	if (!q->fwd_desc && !q->fwd_build)
		return 0;
	fqparams_fill(c, &fq, q->d_fdesc, q->d_fscratch, q->nb, q->fwd_tiles, q->compact ? 8u : 16u, q->fwd_nrings);
	fq.cap_units = q->fwd_cap_units;
	HIPCHK(hipSetDevice(c->device));
	fwd_mark_used(c);
	if (q->fwd_desc) {
		mosrx_dqparams dq;
		memset(&dq, 0, sizeof(dq));
		dq.desc = q->d_ddesc;
		dq.tab = fq.tab;
		dq.scratch = fq.scratch;
		dq.nb = fq.nb;
		dq.total_tiles = fq.total_tiles;
		dq.nrings = fq.nrings;
		rc = mosrx_launch_fwd_desc_queue_build(&fq, &dq, (void *)s);
	} else
		rc = mosrx_launch_fwd_queue_build(&fq, (void *)s);
	mosrx__note_stream(c, s);
	return rc;
}

/* What either attach asks of batch i whatever its outputs are: an input netdev
 * in range and, of a batch with frames, its plan array and off[] / len[]
 * aligned to the kernels' loads. */
static int queue_batch_ok(const mosrx_queue *q, uint32_t i, const uint8_t *in_ifidx, mosrx_fwd *const *d_plan)
{
	const mosrx_qdesc *d = &q->h_desc[i];
	if (in_ifidx && in_ifidx[i] >= MOSRX_FWD_MAX_NETDEVS)
		return 0;
	return !d->n || (aligned(d_plan[i], 8) && !((uintptr_t)d->off & 3) && !((uintptr_t)d->len & 1));
}

/* The queue's scratch rows only grow: an attach that needs no more keeps them. */
static int queue_scratch_reserve(mosrx_queue *q, size_t rows)
{
	if (rows <= q->fscratch_rows)
		return 0;
	if (q->d_fscratch)
		hipFree(q->d_fscratch);
	q->d_fscratch = NULL;
	q->fscratch_rows = 0;
	if (hipMalloc((void **)&q->d_fscratch, rows * MOSRX_FWD_ROW) != hipSuccess)
		return -ENOMEM;
	q->fscratch_rows = rows;
	return 0;
}

/* A queue's device table, allocated at the first attach that fills it. */
static int queue_table_upload(void **d_tab, const void *h, size_t bytes)
{
	if (!*d_tab && hipMalloc(d_tab, bytes) != hipSuccess)
		return -ENOMEM;
	return hipMemcpy(*d_tab, h, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -EIO;
}

int mosrx_queue_set_fwd(mosrx_ctx *c, mosrx_queue *q, const mosrx_queue_fwd *f)
{
	mosrx_fdesc *h;
	uint32_t i, tiles = 0;
	int build, rc;
	if (!c || !q)
		return -EINVAL;
	if (!f) {
		if (!q->fwd_desc)   /* (the descriptor form is detached by its own call) */
			q->fwd = q->fwd_build = 0;
		return 0;
	}
	if (q->fwd_desc)
		return -EINVAL;
	build = f->d_tx_frames || f->d_tx_off || f->d_tx_len || f->d_tx_src || f->d_rings;
	if (!f->d_plan || (build && (!f->d_tx_frames || !f->d_tx_off || !f->d_tx_len || !f->d_tx_src || !f->d_rings ||
	                             !ring_cap_ok(f->ring_cap, f->nrings))))
		return -EINVAL;
	for (i = 0; i < q->nb; i++)
		if (!queue_batch_ok(q, i, f->in_ifidx, f->d_plan) ||
		    (build && !ring_out_ok(q->h_desc[i].n != 0, f->d_tx_frames[i], f->d_tx_off[i], f->d_tx_len[i], f->d_tx_src[i],
		                           f->d_rings[i])))
			return -EINVAL;
	if (!(h = calloc(q->nb, sizeof(*h))))
		return -ENOMEM;
	for (i = 0; i < q->nb; i++) {
		tiles += fdesc_fill(&h[i], &q->h_desc[i], f->in_ifidx ? f->in_ifidx[i] : 0, tiles, f->d_plan[i],
		                    build ? f->d_rings[i] : NULL);
		if (build && h[i].n) {
			h[i].tx = f->d_tx_frames[i];
			h[i].tx_off = f->d_tx_off[i];
			h[i].tx_len = f->d_tx_len[i];
			h[i].tx_src = f->d_tx_src[i];
		}
	}
	/* from here a failure leaves the queue without forwarding */
	q->fwd = q->fwd_build = 0;
	rc = hipSetDevice(c->device) == hipSuccess ? 0 : -EIO;
	if (!rc)
		rc = queue_scratch_reserve(q, build ? ((size_t)tiles ? tiles : 1) * f->nrings : 0);
	if (!rc)
		rc = queue_table_upload((void **)&q->d_fdesc, h, (size_t)q->nb * sizeof(*h));
	free(h);
	if (rc)
		return rc;
	q->fwd_tiles = tiles;
	q->fwd_nrings = build ? f->nrings : 0;
	q->fwd_cap_units = build ? (uint32_t)(f->ring_cap / 16) : 0;
	q->fwd_build = build;
	q->fwd = 1;
	return 0;
}

int mosrx_queue_set_fwd_desc(mosrx_ctx *c, mosrx_queue *q, const mosrx_queue_fwd_desc *f)
{
	mosrx_fdesc *h;
	mosrx_ddesc *g;
	uint32_t i, tiles = 0, maxn = 0;
	int rc;
	if (!c || !q)
		return -EINVAL;
	if (!f) {
		if (q->fwd_desc)
			q->fwd = q->fwd_desc = 0;
		return 0;
	}
	if (q->fwd && !q->fwd_desc)   /* mosrx_queue_set_fwd's attachment is in place */
		return -EINVAL;
	if (!f->d_plan || !f->d_tx_src || !f->d_tx_len || !f->d_tx_mac || !f->d_rings || !nrings_ok(f->nrings))
		return -EINVAL;
	for (i = 0; i < q->nb; i++)
		if (!queue_batch_ok(q, i, f->in_ifidx, f->d_plan) ||
		    !desc_out_ok(q->h_desc[i].n != 0, f->d_tx_src[i], f->d_tx_len[i], f->d_tx_mac[i], f->d_rings[i], 16))
			return -EINVAL;
	h = calloc(q->nb, sizeof(*h));
	g = calloc(q->nb, sizeof(*g));
	if (!h || !g) {
		free(h);
		free(g);
		return -ENOMEM;
	}
	for (i = 0; i < q->nb; i++) {
		tiles += fdesc_fill(&h[i], &q->h_desc[i], f->in_ifidx ? f->in_ifidx[i] : 0, tiles, f->d_plan[i], f->d_rings[i]);
		ddesc_from(&g[i], &h[i], f->d_tx_src[i], f->d_tx_len[i], f->d_tx_mac[i]);
		if (h[i].n > maxn)
			maxn = h[i].n;
	}
	/* from here a failure leaves the queue without forwarding, as mosrx_queue_set_fwd's does */
	q->fwd = q->fwd_build = q->fwd_desc = 0;
	rc = hipSetDevice(c->device) == hipSuccess ? 0 : -EIO;
	if (!rc)
		rc = queue_scratch_reserve(q, ((size_t)tiles ? tiles : 1) * f->nrings);
	if (!rc)
		rc = queue_table_upload((void **)&q->d_fdesc, h, (size_t)q->nb * sizeof(*h));
	if (!rc)
		rc = queue_table_upload((void **)&q->d_ddesc, g, (size_t)q->nb * sizeof(*g));
	free(h);
	free(g);
	if (rc)
		return rc;
	q->fwd_tiles = tiles;
	q->fwd_nrings = f->nrings;
	q->fwd_cap_units = 0;
	q->fwd_maxn = maxn;
	q->fwd_desc = 1;
	q->fwd = 1;
	return 0;
}

/* ---- forwarding of a group (mosrx_slot_fwd) ----------------------------------------- */

int mosrx_slot_fwd(mosrx_ctx *c, int slot, const mosrx_slot_fwd_out *o)
{
	int rc;
	if (!c || slot < 0 || slot >= NSLOT)
		return -EINVAL;
	if (c->slot[slot].busy)
		return -EBUSY;
	if (!o) {
		c->slot[slot].fwd_armed = 0;
		return 0;
	}
	if (!o->h_tx_src || !o->h_tx_len || !o->h_tx_mac || !o->h_rings || !nrings_ok(o->nrings))
		return -EINVAL;
	if ((rc = mosrx__fwd_group_check(c, o)))
		return rc;
	c->slot[slot].fwd = *o;
	c->slot[slot].fwd_armed = 1;
	return 0;
}

int mosrx__fwd_group_check(const mosrx_ctx *c, const mosrx_slot_fwd_out *o)
{
	if (!c->d_fwd)
		return -ENOENT;
	if (o->nrings < c->fwd_num_netdevs)
		return -EINVAL;
	return 0;
}

int mosrx__fwd_group_check_batch(const mosrx_slot_fwd_out *o, uint32_t i, uint32_t n)
{
	/* rings to 4 bytes, not the kernels' 16: rows aligned to less are not written
	 * in place (mosrx__fwd_group_outputs) but copied back from the slot's own */
	if ((o->in_ifidx && o->in_ifidx[i] >= MOSRX_FWD_MAX_NETDEVS) ||
	    !desc_out_ok(n != 0, o->h_tx_src[i], o->h_tx_len[i], o->h_tx_mac[i], o->h_rings[i], 4) ||
	    (n && o->h_plan && !aligned(o->h_plan[i], 8)))
		return -EINVAL;
	return 0;
}

void mosrx__fwd_group_empty(const mosrx_slot_fwd_out *o, uint32_t nb)
{
	uint32_t i;
	for (i = 0; i < nb; i++)
		memset(o->h_rings[i], 0, (size_t)o->nrings * sizeof(mosrx_fwd_ring));
}

int mosrx__fwd_group_outputs(int device, const mosrx_batch *b, uint32_t nb, const mosrx_slot_fwd_out *o, mosrx_fdesc *fd,
                             mosrx_ddesc *dd)
{
	uint32_t i;
	for (i = 0; i < nb; i++) {
		const uint64_t n = b[i].n;
		if (!aligned(o->h_rings[i], 16) ||
		    !(dd[i].rings = mosrx__host_dev_of(o->h_rings[i], (uint64_t)o->nrings * sizeof(mosrx_fwd_ring), device)))
			return 0;
		fd[i].rings = dd[i].rings;
		if (!n)
			continue;
		fd[i].plan = NULL;   /* (no h_plan: the slot's own array) */
		if (o->h_plan && !(fd[i].plan = mosrx__host_dev_of(o->h_plan[i], n * sizeof(mosrx_fwd), device)))
			return 0;
		if (!(dd[i].tx_src = mosrx__host_dev_of(o->h_tx_src[i], n * 4, device)) ||
		    !(dd[i].tx_len = mosrx__host_dev_of(o->h_tx_len[i], n * 2, device)) ||
		    !(dd[i].tx_mac = mosrx__host_dev_of(o->h_tx_mac[i], n * 12, device)))
			return 0;
	}
	return 1;
}

int mosrx__fwd_group_launch_acl(mosrx_ctx *c, struct slot *s, const mosrx_batch *b, uint32_t nb, size_t rsz, int in_place,
                                const mosrx_slot_fwd_out *o, uint16_t *const *h_hit, uint32_t *h_counts)
{
	mosrx_fqparams fq;
	uint32_t i, tiles = 0, maxn = 0;
	uint64_t pre = 0;
	int rc;
	for (i = 0; i < nb; pre += b[i].n, i++) {
		mosrx_fdesc *f = &s->h_fdesc[i];
		mosrx_ddesc *d = &s->h_ddesc[i];
		/* in place, the tables hold the caller's arrays where it gave them; the rest is the slot's */
		mosrx_fwd *const plan = in_place && b[i].n && f->plan ? f->plan : s->d_fplan + pre;
		tiles += fdesc_fill(f, &s->h_qdesc[i], o->in_ifidx ? o->in_ifidx[i] : 0, tiles, plan,
		                    in_place ? d->rings : s->d_frings + (size_t)i * MOSRX_FWD_MAX_NETDEVS);
		if (in_place)
			ddesc_from(d, f, d->tx_src, d->tx_len, d->tx_mac);
		else
			ddesc_from(d, f, s->d_ftsrc + pre, s->d_ftlen + pre, s->d_ftmac + 3 * pre);
		if (b[i].n > maxn)
			maxn = b[i].n;
	}
	HIPCHK(hipMemcpyAsync(s->d_fdesc, s->h_fdesc, nb * sizeof(mosrx_fdesc), hipMemcpyHostToDevice, s->stream));
	HIPCHK(hipMemcpyAsync(s->d_ddesc, s->h_ddesc, nb * sizeof(mosrx_ddesc), hipMemcpyHostToDevice, s->stream));
	fqparams_fill(c, &fq, s->d_fdesc, s->d_fscr, nb, tiles, (uint32_t)rsz, o->nrings);
	fwd_mark_used(c);
	if (!h_hit) {
		if ((rc = fwd_desc_queue_launch(c, &fq, s->d_ddesc, maxn, (void *)s->stream)))
			return rc;
	} else {
		/* the firewall launch between the plan and the build: never the one-launch form */
		mosrx_dqparams dq;
		memset(&dq, 0, sizeof(dq));
		dq.desc = s->d_ddesc;
		dq.tab = fq.tab;
		dq.scratch = fq.scratch;
		dq.nb = fq.nb;
		dq.total_tiles = fq.total_tiles;
		dq.nrings = fq.nrings;
		if ((rc = mosrx_launch_fwd_queue(&fq, 0, (void *)s->stream)) ||
		    (rc = mosrx__acl_group_launch(c, s, b, nb, rsz, in_place, 1, h_hit, h_counts)) ||
		    (rc = mosrx_launch_fwd_desc_queue_build(&fq, &dq, (void *)s->stream)))
			return rc;
	}
	for (i = 0, pre = 0; i < nb; pre += b[i].n, i++) {
		const size_t n = b[i].n;
		if (o->h_plan && n && s->h_fdesc[i].plan == s->d_fplan + pre)
			HIPCHK(hipMemcpyAsync(o->h_plan[i], s->d_fplan + pre, n * sizeof(mosrx_fwd), hipMemcpyDeviceToHost, s->stream));
		if (in_place)
			continue;
		HIPCHK(hipMemcpyAsync(o->h_rings[i], s->d_frings + (size_t)i * MOSRX_FWD_MAX_NETDEVS,
		                      (size_t)o->nrings * sizeof(mosrx_fwd_ring), hipMemcpyDeviceToHost, s->stream));
		if (!n)
			continue;
		HIPCHK(hipMemcpyAsync(o->h_tx_src[i], s->d_ftsrc + pre, n * 4, hipMemcpyDeviceToHost, s->stream));
		HIPCHK(hipMemcpyAsync(o->h_tx_len[i], s->d_ftlen + pre, n * 2, hipMemcpyDeviceToHost, s->stream));
		HIPCHK(hipMemcpyAsync(o->h_tx_mac[i], s->d_ftmac + 3 * pre, n * 12, hipMemcpyDeviceToHost, s->stream));
	}
	return 0;
}

int mosrx__fwd_group_launch(mosrx_ctx *c, struct slot *s, const mosrx_batch *b, uint32_t nb, size_t rsz, int in_place,
                            const mosrx_slot_fwd_out *o)
{
	return mosrx__fwd_group_launch_acl(c, s, b, nb, rsz, in_place, o, NULL, NULL);
}

/* ---- the timing ops (mosrx_time_op) ------------------------------------------------- */

#define TMP_RND(x) (((size_t)(x) + 255) & ~(size_t)255)

/* The block's layout: one for the context stream and one per timing stream,
 * sized for the largest batch (each part rounded to 256 bytes): tx_frames as
 * `nrings` rings (MOSRX_OP_FWD: one), each with room for every frame of the
 * batch sent whole (its frame bytes + 32 a frame; the rings together at most
 * 4 GiB), tx_off, tx_src, tx_len, tx_nif, tx_count / the ring rows, scratch.
 * MOSRX_OP_FWD_DESC takes the same block: its tx_mac (12 bytes an entry) lies
 * where the rings would (each has room for 32 bytes a frame).  MOSRX_OP_FWD_NAT
 * takes MOSRX_OP_FWD_RINGS' block with its xlat array (16 bytes a frame) behind
 * the scratch. */
int mosrx__fwd_tmp_reserve(mosrx_ctx *c, int op, const mosrx_batch *b, uint32_t nb)
{
	const uint32_t nrings = op == MOSRX_OP_FWD || !c->fwd_num_netdevs ? 1 : c->fwd_num_netdevs;
	uint32_t i, maxn = 0;
	uint64_t maxb = 0, cap;
	size_t stride, bytes;
	if (op == MOSRX_OP_FWD_PLAN)
		return 0;
	if (op != MOSRX_OP_FWD && !c->d_fwd)   /* the ring ops */
		return -ENOENT;
	for (i = 0; i < nb; i++) {
		maxn = b[i].n > maxn ? b[i].n : maxn;
		maxb = b[i].frames_bytes > maxb ? b[i].frames_bytes : maxb;
	}
	cap = TMP_RND(maxb + 32ull * maxn);
	if (nrings > 1 && cap > ((1ull << 32) / nrings & ~255ull))
		cap = (1ull << 32) / nrings & ~255ull;
	c->fwd_tmp_n = maxn;
	c->fwd_tmp_cap = cap;
	c->fwd_tmp_rings = nrings;
	stride = c->fwd_tmp_cap * nrings + 2 * TMP_RND((size_t)maxn * 4) + TMP_RND((size_t)maxn * 2) + TMP_RND(maxn) + 256 +
	         TMP_RND(mosrx_fwd_rings_scratch_bytes(maxn, nrings)) +
	         (op == MOSRX_OP_FWD_NAT ? TMP_RND((size_t)maxn * sizeof(mosrx_nat_xlat)) : 0);
	bytes = stride * (MOSRX_MAX_STREAMS + 1);
	if (bytes > c->fwd_tmp_bytes) {
		HIPCHK(hipDeviceSynchronize());
		if (c->fwd_tmp)
			hipFree(c->fwd_tmp);
		c->fwd_tmp = NULL;
		c->fwd_tmp_bytes = 0;
		if (hipMalloc((void **)&c->fwd_tmp, bytes) != hipSuccess)
			return -ENOMEM;
		c->fwd_tmp_bytes = bytes;
	}
	c->fwd_tmp_stride = stride;
	return 0;
}

int mosrx__fwd_op(mosrx_ctx *c, int op, int arg, const mosrx_batch *b, void *out, void *aux, hipStream_t s)
{
	uint32_t k = 0;
	uint8_t *blk, *toff, *tsrc, *tlen, *tnif, *tcnt, *scr;
	const size_t w = TMP_RND((size_t)c->fwd_tmp_n * 4);
	/* the descriptor form under mosrx_set_fwd_one's limit: plan and rings in one launch, below */
	const int one = op == MOSRX_OP_FWD_DESC && c->fwd_one && b->n <= c->fwd_one;
	int rc = one || op == MOSRX_OP_FWD_NAT ? 0 : mosrx_fwd_plan_dev(c, b, out, arg & 0xFF, arg >> 8, (mosrx_fwd *)aux, s);
	if (rc || op == MOSRX_OP_FWD_PLAN)
		return rc;
	/* the stream's own block: launches on different streams overlap */
	while (k < c->nxs && c->xs[k] != s)
		k++;
	blk = c->fwd_tmp + (size_t)(k < c->nxs ? k + 1 : 0) * c->fwd_tmp_stride;
	toff = blk + c->fwd_tmp_cap * c->fwd_tmp_rings;
	tsrc = toff + w;
	tlen = tsrc + w;
	tnif = tlen + TMP_RND((size_t)c->fwd_tmp_n * 2);
	tcnt = tnif + TMP_RND(c->fwd_tmp_n);
	scr = tcnt + 256;
	if (one)
		return fwd_plan_desc_one(c, b, out, arg & 0xFF, arg >> 8, (mosrx_fwd *)aux, c->fwd_tmp_rings, (uint32_t *)tsrc,
		                         (uint16_t *)tlen, (uint32_t *)blk, (mosrx_fwd_ring *)tcnt, scr,
		                         TMP_RND(mosrx_fwd_desc_scratch_bytes(c->fwd_tmp_n, c->fwd_tmp_rings)), s);
	if (op == MOSRX_OP_FWD_DESC)
		return mosrx_fwd_desc_rings_dev(c, b, (const mosrx_fwd *)aux, c->fwd_tmp_rings, (uint32_t *)tsrc, (uint16_t *)tlen,
		                                (uint32_t *)blk, (mosrx_fwd_ring *)tcnt, scr,
		                                TMP_RND(mosrx_fwd_desc_scratch_bytes(c->fwd_tmp_n, c->fwd_tmp_rings)), s);
	if (op == MOSRX_OP_FWD_NAT) {
		/* plan-nat in the plan's place, the ring build, the patch; the xlat array behind the scratch */
		mosrx_nat_xlat *xl = (mosrx_nat_xlat *)(scr + TMP_RND(mosrx_fwd_rings_scratch_bytes(c->fwd_tmp_n, c->fwd_tmp_rings)));
		if ((rc = mosrx_fwd_plan_nat_dev(c, b, out, arg & 0xFF, arg >> 8, (mosrx_fwd *)aux, xl, s)) ||
		    (rc = mosrx_fwd_build_rings_dev(c, b, (const mosrx_fwd *)aux, blk, c->fwd_tmp_cap, c->fwd_tmp_rings,
		                                    (uint32_t *)toff, (uint16_t *)tlen, (uint32_t *)tsrc, (mosrx_fwd_ring *)tcnt, scr,
		                                    TMP_RND(mosrx_fwd_rings_scratch_bytes(c->fwd_tmp_n, c->fwd_tmp_rings)), s)))
			return rc;
		return mosrx_nat_patch_rings_dev(c, xl, blk, (const uint32_t *)toff, (const uint32_t *)tsrc,
		                                 (const mosrx_fwd_ring *)tcnt, c->fwd_tmp_rings, b->n, s);
	}
	if (op == MOSRX_OP_FWD_RINGS)
		return mosrx_fwd_build_rings_dev(c, b, (const mosrx_fwd *)aux, blk, c->fwd_tmp_cap, c->fwd_tmp_rings,
		                                 (uint32_t *)toff, (uint16_t *)tlen, (uint32_t *)tsrc, (mosrx_fwd_ring *)tcnt, scr,
		                                 TMP_RND(mosrx_fwd_rings_scratch_bytes(c->fwd_tmp_n, c->fwd_tmp_rings)), s);
	return mosrx_fwd_build_dev(c, b, (const mosrx_fwd *)aux, blk, c->fwd_tmp_cap, (uint32_t *)toff, (uint16_t *)tlen,
	                           (int8_t *)tnif, (uint32_t *)tsrc, (uint32_t *)tcnt, scr,
	                           TMP_RND(mosrx_fwd_scratch_bytes(c->fwd_tmp_n)), s);
}
