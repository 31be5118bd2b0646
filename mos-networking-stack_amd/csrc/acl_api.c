/*
 * acl_api.c — host side of the firewall rules (include/mosrx.h; kernel in mosrx_acl.hip).
 *
 * The rule table, the single-batch call and the batch-queue attachment, their
 * argument refusals and their one launch.  mosrx_api.c keeps the flows they
 * hang on (the queue run, the timing ops, the queue's release) and reaches this
 * file through the mosrx__acl_* functions of mosrx_ctx.h.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "mosrx_ctx.h"

/* non-NULL and aligned to a (a power of two) */
static int aligned(const void *p, uintptr_t a)
{
	return p && !((uintptr_t)p & (a - 1));
}

static uint32_t acl_tiles(uint32_t n)
{
	return (uint32_t)(((size_t)n + MOSRX_ACL_TILE - 1) / MOSRX_ACL_TILE);
}

/* ---- the context's rules --------------------------------------------------------- */

int mosrx_acl_check(const mosrx_acl_rule *rules, uint32_t n)
{
	uint32_t i;
	if (n > MOSRX_ACL_MAX_RULES || (n && !rules))
		return -EINVAL;
	for (i = 0; i < n; i++)
		if (rules[i].action != MOSRX_ACL_ACCEPT && rules[i].action != MOSRX_ACL_DROP)
			return -EINVAL;
	return 0;
}

uint32_t mosrx_acl_count(const mosrx_ctx *c) { return c ? c->acl_n : 0; }

/* The rules go to the next buffer of a pool, as the forwarding tables do
 * (fwd_api.c mosrx_fwd_set): launches submitted earlier may still read the copy
 * they were given, so a buffer is written again only after those launches
 * drained, and only if a launch may have read it since its last write. */
int mosrx_acl_set(mosrx_ctx *c, const mosrx_acl_rule *rules, uint32_t n)
{
	mosrx_acl_dev *h;
	uint32_t i, k;
	int rc;
	if (!c)
		return -EINVAL;
	if (!rules || !n) {
		if (n)
			return -EINVAL;
		c->d_acl = NULL;
		c->acl_n = 0;
		return 0;
	}
	if ((rc = mosrx_acl_check(rules, n)))
		return rc;
	if (!(h = calloc(1, sizeof(*h))))
		return -ENOMEM;
	h->n = n;
	for (i = 0; i < n; i++) {
		const mosrx_acl_rule *r = &rules[i];
		/* MatchAddr (simple_firewall.c:291-298): fw_ip == 0 || (ip & mask) == fw_ip */
		h->src_ip[i] = r->src_ip;
		h->src_mask[i] = r->src_ip ? r->src_mask : 0;
		h->dst_ip[i] = r->dst_ip;
		h->dst_mask[i] = r->dst_ip ? r->dst_mask : 0;
		/* MatchPort (:300-305): fw_port == 0 || port == fw_port, both sides in one dword */
		h->ports[i] = (uint32_t)r->sport | (uint32_t)r->dport << 16;
		h->port_mask[i] = (r->sport ? 0xFFFFu : 0u) | (r->dport ? 0xFFFF0000u : 0u);
		h->action[i] = r->action;
	}
	rc = 0;
	k = c->acl_pool_next;
	if (hipSetDevice(c->device) != hipSuccess)
		rc = -EIO;
	if (!rc && !c->d_acl_pool[k] && hipMalloc((void **)&c->d_acl_pool[k], sizeof(*h)) != hipSuccess)
		rc = -ENOMEM;
	if (!rc && c->acl_pool_used[k] && !(rc = mosrx__drain(c)))
		memset(c->acl_pool_used, 0, sizeof(c->acl_pool_used));
	if (!rc && hipMemcpy(c->d_acl_pool[k], h, sizeof(*h), hipMemcpyHostToDevice) != hipSuccess)
		rc = -EIO;
	free(h);
	if (rc)
		return rc;
	c->d_acl = c->d_acl_pool[k];
	c->acl_n = n;
	c->acl_pool_next = (k + 1) % MOSRX_ACL_POOL;
	return 0;
}

void mosrx__acl_free(mosrx_ctx *c)
{
	uint32_t i;
	for (i = 0; i < MOSRX_ACL_POOL; i++)
		if (c->d_acl_pool[i])
			hipFree(c->d_acl_pool[i]);
}

/* A launch that reads the installed rules is about to go to stream. */
static void acl_mark_used(mosrx_ctx *c)
{
	c->acl_pool_used[(c->acl_pool_next + MOSRX_ACL_POOL - 1) % MOSRX_ACL_POOL] = 1;
}

/* What the launch takes from the context: the installed rules and the
 * parameters of mosrx_mos_forwards' TCP arm. */
static void acl_ctx_params(const mosrx_ctx *c, mosrx_aparams *ap)
{
	memset(ap, 0, sizeof(*ap));
	ap->tab = c->d_acl;
	ap->forward = c->params.forward;
	ap->num_msp = c->params.num_msp;
	ap->listener = c->fwd_listener;
}

/* ---- one device-resident batch --------------------------------------------------- */

int mosrx_acl_apply_dev(mosrx_ctx *c, const mosrx_batch *b, const void *d_rec, int rec_bytes, mosrx_fwd *d_plan,
                        uint16_t *d_hit, uint32_t *d_counts, void *stream)
{
	mosrx_aparams ap;
	hipStream_t s;
	int rc;
	if (!c || !b || (rec_bytes != 8 && rec_bytes != 16) || !aligned(d_hit, 2) || (d_plan && !aligned(d_plan, 8)) ||
	    (d_counts && !aligned(d_counts, 4)) || (b->n && !aligned(d_rec, (uintptr_t)rec_bytes)))
		return -EINVAL;
	if ((rc = mosrx__check_batch(b, 1)))
		return rc;
	if (b->n && ((((uintptr_t)b->off) & 3) || (((uintptr_t)b->len) & 1)))
		return -EINVAL;
	if (!c->d_acl)
		return -ENOENT;
	if (b->n == 0)
		return 0;
	acl_ctx_params(c, &ap);
	ap.frames = b->frames;
	ap.off = b->off;
	ap.len = b->len;
	ap.rec = (const uint8_t *)d_rec;
	ap.plan = d_plan;
	ap.hit = d_hit;
	ap.counts = d_counts;
	ap.frames_bytes = (uint32_t)b->frames_bytes;
	ap.n = b->n;
	ap.rec_bytes = (uint32_t)rec_bytes;
	s = stream ? (hipStream_t)stream : c->stream;
	HIPCHK(hipSetDevice(c->device));
	acl_mark_used(c);
	rc = mosrx_launch_acl(&ap, (void *)s);
	mosrx__note_stream(c, s);   /* (after the launch: its event covers it) */
	return rc;
}

/* ---- over a batch queue (mosrx_queue_set_acl) -------------------------------------- */

int mosrx__acl_queue_check(const mosrx_ctx *c, const mosrx_queue *q)
{
	(void)q;
	return c->d_acl ? 0 : -ENOENT;
}

int mosrx__acl_queue_launch(mosrx_ctx *c, const mosrx_queue *q, int with_plan, void *stream)
{
	mosrx_aparams ap;
	const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	int rc;
	acl_ctx_params(c, &ap);
	ap.adesc = q->d_adesc;
	ap.fdesc = with_plan ? q->d_fdesc : NULL;
	ap.counts = q->acl_counts;
	ap.nb = q->nb;
	ap.total_tiles = q->acl_tiles;
	ap.rec_bytes = q->compact ? 8u : 16u;
	HIPCHK(hipSetDevice(c->device));
	acl_mark_used(c);
	rc = mosrx_launch_acl(&ap, (void *)s);
	mosrx__note_stream(c, s);
	return rc;
}

int mosrx_queue_set_acl(mosrx_ctx *c, mosrx_queue *q, uint16_t *const *d_hit, uint32_t *d_counts)
{
	mosrx_adesc *h;
	uint32_t i, tiles = 0;
	int rc;
	if (!c || !q)
		return -EINVAL;
	if (!d_hit) {
		q->acl = 0;
		return 0;
	}
	if (d_counts && !aligned(d_counts, 4))
		return -EINVAL;
	for (i = 0; i < q->nb; i++) {
		const mosrx_qdesc *d = &q->h_desc[i];
		if (d->n && (!aligned(d_hit[i], 2) || ((uintptr_t)d->off & 3) || ((uintptr_t)d->len & 1)))
			return -EINVAL;
	}
	if (!(h = calloc(q->nb, sizeof(*h))))
		return -ENOMEM;
	/* tile_base[] as fdesc_fill (fwd_api.c) builds it: the same tile, the same order */
	for (i = 0; i < q->nb; i++) {
		const mosrx_qdesc *d = &q->h_desc[i];
		h[i].n = d->n;
		h[i].tile_base = tiles;
		if (d->n) {
			h[i].frames = d->frames;
			h[i].off = d->off;
			h[i].len = d->len;
			h[i].rec = (const uint8_t *)d->out;
			h[i].hit = d_hit[i];
			h[i].frames_bytes = d->frames_bytes;
		}
		tiles += acl_tiles(d->n);
	}
	/* from here a failure leaves the queue without the attachment */
	q->acl = 0;
	rc = hipSetDevice(c->device) == hipSuccess ? 0 : -EIO;
	if (!rc && !q->d_adesc && hipMalloc((void **)&q->d_adesc, (size_t)q->nb * sizeof(*h)) != hipSuccess)
		rc = -ENOMEM;
	/* (a run of this queue submitted earlier may still read the table) */
	if (!rc)
		rc = mosrx__drain(c);
	if (!rc && hipMemcpy(q->d_adesc, h, (size_t)q->nb * sizeof(*h), hipMemcpyHostToDevice) != hipSuccess)
		rc = -EIO;
	free(h);
	if (rc)
		return rc;
	q->acl_tiles = tiles;
	q->acl_counts = d_counts;
	q->acl = 1;
	return 0;
}

/* ---- the firewall launch of a group (mosrx_slot_acl) --------------------------------- */

int mosrx_slot_acl(mosrx_ctx *c, int slot, uint16_t *const *h_hit, uint32_t *h_counts)
{
	if (!c || slot < 0 || slot >= NSLOT)
		return -EINVAL;
	if (c->slot[slot].busy)
		return -EBUSY;
	if (!h_hit) {
		c->slot[slot].acl_armed = 0;
		return 0;
	}
	if (h_counts && !aligned(h_counts, 4))
		return -EINVAL;
	if (!c->d_acl)
		return -ENOENT;
	c->slot[slot].acl_hit = h_hit;
	c->slot[slot].acl_counts = h_counts;
	c->slot[slot].acl_armed = 1;
	return 0;
}

int mosrx__acl_group_check(const mosrx_ctx *c)
{
	return c->d_acl ? 0 : -ENOENT;
}

int mosrx__acl_group_check_batch(uint16_t *const *h_hit, uint32_t i, uint32_t n)
{
	return n && !aligned(h_hit[i], 2) ? -EINVAL : 0;
}

int mosrx__acl_group_outputs(int device, struct slot *s, const mosrx_batch *b, uint32_t nb, uint16_t *const *h_hit)
{
	uint32_t i;
	for (i = 0; i < nb; i++) {
		s->h_adesc[i].hit = NULL;
		if (b[i].n && !(s->h_adesc[i].hit = mosrx__host_dev_of(h_hit[i], (uint64_t)b[i].n * 2, device)))
			return 0;
	}
	return 1;
}

int mosrx__acl_group_launch(mosrx_ctx *c, struct slot *s, const mosrx_batch *b, uint32_t nb, size_t rsz, int in_place,
                            int with_plan, uint16_t *const *h_hit, uint32_t *h_counts)
{
	mosrx_aparams ap;
	uint32_t i, tiles = 0;
	uint64_t pre = 0;
	uint32_t *cnt = NULL;
	int rc;
	/* tile_base[] as fdesc_fill (fwd_api.c) builds it: the same tile, the same order */
	for (i = 0; i < nb; pre += b[i].n, i++) {
		const mosrx_qdesc *d = &s->h_qdesc[i];
		mosrx_adesc *a = &s->h_adesc[i];
		uint16_t *const hit = in_place ? a->hit : s->d_ahit + pre;
		memset(a, 0, sizeof(*a));
		a->n = d->n;
		a->tile_base = tiles;
		if (d->n) {
			a->frames = d->frames;
			a->off = d->off;
			a->len = d->len;
			a->rec = (const uint8_t *)d->out;
			a->hit = hit;
			a->frames_bytes = d->frames_bytes;
		}
		tiles += acl_tiles(d->n);
	}
	HIPCHK(hipMemcpyAsync(s->d_adesc, s->h_adesc, nb * sizeof(mosrx_adesc), hipMemcpyHostToDevice, s->stream));
	/* the counts: the caller's array where the device reaches it, else a copy in and out */
	if (h_counts && !(cnt = mosrx__host_dev_of(h_counts, MOSRX_ACL_MAX_RULES * 4, c->device))) {
		cnt = s->d_acnt;
		HIPCHK(hipMemcpyAsync(cnt, h_counts, MOSRX_ACL_MAX_RULES * 4, hipMemcpyHostToDevice, s->stream));
	}
	acl_ctx_params(c, &ap);
	ap.adesc = s->d_adesc;
	ap.fdesc = with_plan ? s->d_fdesc : NULL;
	ap.counts = cnt;
	ap.nb = nb;
	ap.total_tiles = tiles;
	ap.rec_bytes = (uint32_t)rsz;
	acl_mark_used(c);
	if ((rc = mosrx_launch_acl(&ap, (void *)s->stream)))
		return rc;
	if (cnt == s->d_acnt)
		HIPCHK(hipMemcpyAsync(h_counts, cnt, MOSRX_ACL_MAX_RULES * 4, hipMemcpyDeviceToHost, s->stream));
	for (i = 0, pre = 0; !in_place && i < nb; pre += b[i].n, i++)
		if (b[i].n)
			HIPCHK(hipMemcpyAsync(h_hit[i], s->d_ahit + pre, (size_t)b[i].n * 2, hipMemcpyDeviceToHost, s->stream));
	return 0;
}
