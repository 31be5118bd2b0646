/*
 * nat_api.c — host side of NAT translation (include/mosrx.h; kernels in mosrx_nat.hip).
 *
 * The binding table (validated and built here, on the host), the plan-nat and
 * patch calls, the batch-queue attachment, their argument refusals and their
 * launches.  mosrx_api.c keeps the flows they hang on (the queue run, the timing
 * ops, the queue's release) and reaches this file through the mosrx__nat_*
 * functions of mosrx_ctx.h.
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

/* ---- the table ------------------------------------------------------------------- */

uint32_t mosrx_nat_hash(uint32_t saddr, uint32_t daddr, uint32_t ports)
{
	return mosrx_nat_hash_key(saddr, daddr, ports);
}

uint32_t mosrx_nat_slots(uint32_t n)
{
	uint32_t cap = MOSRX_NAT_MIN_SLOTS;
	if (n > MOSRX_NAT_MAX_BINDINGS)
		n = MOSRX_NAT_MAX_BINDINGS;
	while (cap < 4u * n)
		cap <<= 1;
	return cap;
}

/* One key into the table: 0, or -EINVAL when it is there already.  *probe grows
 * to the slots this key's lookup examines. */
static int nat_insert(mosrx_nat_slot *slots, uint32_t mask, uint32_t sa, uint32_t da, uint32_t pt, uint8_t kind,
                      uint32_t addr, uint16_t port, uint32_t bind, uint32_t *probe)
{
	const uint32_t h = mosrx_nat_hash_key(sa, da, pt);
	uint32_t d;
	for (d = 0; d <= mask; d++) {   /* (at most half full: a free slot comes) */
		mosrx_nat_slot *s = &slots[(h + d) & mask];
		if (!s->kind) {
			s->saddr = sa;
			s->daddr = da;
			s->ports = pt;
			s->port = port;
			s->kind = kind;
			s->addr = addr;
			s->bind = bind;
			if (d + 1 > *probe)
				*probe = d + 1;
			return 0;
		}
		if (s->saddr == sa && s->daddr == da && s->ports == pt)
			return -EINVAL;
	}
	return -EINVAL;
}

int mosrx_nat_build(const mosrx_nat_binding *b, uint32_t n, mosrx_nat_slot *slots, uint32_t *probe)
{
	uint32_t i, run = 0, mask;
	if (n > MOSRX_NAT_MAX_BINDINGS || (n && !b) || !slots)
		return -EINVAL;
	mask = mosrx_nat_slots(n) - 1;
	memset(slots, 0, ((size_t)mask + 1) * sizeof(*slots));
	for (i = 0; i < n; i++) {
		const mosrx_nat_binding *x = &b[i];
		if (!x->nat_ip || !x->nat_port)
			return -EINVAL;
		/* client side: the frame the client sent; server side: the server's answer to the NAT's address */
		if (nat_insert(slots, mask, x->cli_ip, x->svr_ip, (uint32_t)x->cli_port | (uint32_t)x->svr_port << 16,
		               MOSRX_NAT_SNAT, x->nat_ip, x->nat_port, i, &run) ||
		    nat_insert(slots, mask, x->svr_ip, x->nat_ip, (uint32_t)x->svr_port | (uint32_t)x->nat_port << 16,
		               MOSRX_NAT_DNAT, x->cli_ip, x->cli_port, i, &run))
			return -EINVAL;
	}
	if (probe)
		*probe = run;
	return 0;
}

int mosrx_nat_check(const mosrx_nat_binding *b, uint32_t n)
{
	mosrx_nat_slot *slots;
	int rc;
	if (n > MOSRX_NAT_MAX_BINDINGS || (n && !b))
		return -EINVAL;
	if (!(slots = malloc((size_t)mosrx_nat_slots(n) * sizeof(*slots))))
		return -ENOMEM;
	rc = mosrx_nat_build(b, n, slots, NULL);
	free(slots);
	return rc;
}

uint32_t mosrx_nat_count(const mosrx_ctx *c) { return c ? c->nat_n : 0; }

/* The table goes to the next buffer of a pool, as the forwarding tables do
 * (fwd_api.c mosrx_fwd_set): launches submitted earlier may still read the copy
 * they were given, so a buffer is written again (or freed to grow) only after
 * those launches drained, and only if a launch may have read it since its last
 * write. */
int mosrx_nat_set(mosrx_ctx *c, const mosrx_nat_binding *b, uint32_t n)
{
	mosrx_nat_slot *h;
	uint32_t k, probe = 0, cap;
	size_t bytes;
	int rc;
	if (!c || n > MOSRX_NAT_MAX_BINDINGS || (n && !b))
		return -EINVAL;
	if (!b)
		n = 0;
	cap = mosrx_nat_slots(n);
	bytes = (size_t)cap * sizeof(*h);
	if (!(h = malloc(bytes)))
		return -ENOMEM;
	if ((rc = mosrx_nat_build(b, n, h, &probe))) {
		free(h);
		return rc;
	}
	k = c->nat_pool_next;
	if (hipSetDevice(c->device) != hipSuccess)
		rc = -EIO;
	if (!rc && c->nat_pool_used[k] && !(rc = mosrx__drain(c)))
		memset(c->nat_pool_used, 0, sizeof(c->nat_pool_used));
	if (!rc && c->d_nat_pool[k] && c->nat_pool_bytes[k] < bytes) {
		/* (the installed table is another buffer of the pool, or none: k is the oldest) */
		hipFree(c->d_nat_pool[k]);
		c->d_nat_pool[k] = NULL;
		c->nat_pool_bytes[k] = 0;
	}
	if (!rc && !c->d_nat_pool[k]) {
		if (hipMalloc((void **)&c->d_nat_pool[k], bytes) != hipSuccess)
			rc = -ENOMEM;
		else
			c->nat_pool_bytes[k] = bytes;
	}
	if (!rc && hipMemcpy(c->d_nat_pool[k], h, bytes, hipMemcpyHostToDevice) != hipSuccess)
		rc = -EIO;
	free(h);
	if (rc)
		return rc;
	c->d_nat = c->d_nat_pool[k];
	c->nat_n = n;
	c->nat_mask = cap - 1;
	c->nat_probe = probe;
	c->nat_pool_next = (k + 1) % MOSRX_NAT_POOL;
	return 0;
}

void mosrx__nat_free(mosrx_ctx *c)
{
	uint32_t i;
	for (i = 0; i < MOSRX_NAT_POOL; i++)
		if (c->d_nat_pool[i])
			hipFree(c->d_nat_pool[i]);
}

/* A launch that reads the installed table is about to go to stream. */
static void nat_mark_used(mosrx_ctx *c)
{
	c->nat_pool_used[(c->nat_pool_next + MOSRX_NAT_POOL - 1) % MOSRX_NAT_POOL] = 1;
	mosrx__fwd_mark_used(c);
}

/* What plan-nat takes from the context: the installed tables of both kinds and
 * mosrx_mos_forwards' parameters. */
static void nat_ctx_params(const mosrx_ctx *c, mosrx_nparams *np)
{
	memset(np, 0, sizeof(*np));
	np->f.tab = c->d_fwd;
	np->f.forward = c->params.forward;
	np->f.num_msp = c->params.num_msp;
	np->f.listener = c->fwd_listener;
	np->slots = c->d_nat;
	np->mask = c->nat_mask;
	np->probe = c->nat_probe;
}

/* ---- one frame on the host --------------------------------------------------------- */

void mosrx_nat_patch_frame(uint8_t *frame, const mosrx_nat_xlat *x)
{
	uint32_t th;
	int snat;
	if (!frame || !x || (x->kind != MOSRX_NAT_SNAT && x->kind != MOSRX_NAT_DNAT))
		return;
	snat = x->kind == MOSRX_NAT_SNAT;
	th = 14u + 4u * (x->ihl & 0xFu);
	memcpy(frame + 24, &x->ip_check, 2);
	memcpy(frame + (snat ? 26 : 30), &x->addr, 4);
	memcpy(frame + th + (snat ? 0 : 2), &x->port, 2);
	memcpy(frame + th + 16, &x->tcp_check, 2);
}

/* ---- one device-resident batch --------------------------------------------------- */

int mosrx_fwd_plan_nat_dev(mosrx_ctx *c, const mosrx_batch *b, const void *d_rec, int rec_bytes, int in_ifidx,
                           mosrx_fwd *d_plan, mosrx_nat_xlat *d_xlat, void *stream)
{
	mosrx_nparams np;
	hipStream_t s;
	int rc;
	if (!c || !b || !aligned(d_plan, 8) || !aligned(d_xlat, 16) || (rec_bytes != 8 && rec_bytes != 16) || in_ifidx < 0 ||
	    in_ifidx >= MOSRX_FWD_MAX_NETDEVS || (b->n && !aligned(d_rec, (uintptr_t)rec_bytes)))
		return -EINVAL;
	if ((rc = mosrx__check_batch(b, 1)))
		return rc;
	if (b->n && ((((uintptr_t)b->off) & 3) || (((uintptr_t)b->len) & 1)))
		return -EINVAL;
	if (c->params.skip_tcp_csum)
		return -EINVAL;
	if (!c->d_fwd || !c->d_nat)
		return -ENOENT;
	if (b->n == 0)
		return 0;
	nat_ctx_params(c, &np);
	np.f.frames = b->frames;
	np.f.off = b->off;
	np.f.len = b->len;
	np.f.rec = (const uint8_t *)d_rec;
	np.f.plan = d_plan;
	np.f.frames_bytes = (uint32_t)b->frames_bytes;
	np.f.n = b->n;
	np.f.rec_bytes = (uint32_t)rec_bytes;
	np.f.in_ifidx = in_ifidx;
	np.xlat = d_xlat;
	s = stream ? (hipStream_t)stream : c->stream;
	HIPCHK(hipSetDevice(c->device));
	nat_mark_used(c);
	rc = mosrx_launch_nat_plan(&np, (void *)s);
	mosrx__note_stream(c, s);   /* (after the launch: its event covers it) */
	return rc;
}

int mosrx_nat_patch_rings_dev(mosrx_ctx *c, const mosrx_nat_xlat *d_xlat, uint8_t *d_tx_frames, const uint32_t *d_tx_off,
                              const uint32_t *d_tx_src, const mosrx_fwd_ring *d_rings, uint32_t nrings, uint32_t n,
                              void *stream)
{
	mosrx_npatch pp;
	hipStream_t s;
	if (!c || !aligned(d_xlat, 16) || !aligned(d_tx_frames, 16) || !aligned(d_tx_off, 4) || !aligned(d_tx_src, 4) ||
	    !aligned(d_rings, 16) || nrings < 1 || nrings > MOSRX_FWD_MAX_NETDEVS)
		return -EINVAL;
	if (n == 0)
		return 0;
	memset(&pp, 0, sizeof(pp));
	pp.xlat = d_xlat;
	pp.tx = d_tx_frames;
	pp.tx_off = d_tx_off;
	pp.tx_src = d_tx_src;
	pp.rings = d_rings;
	pp.nrings = nrings;
	pp.n = n;
	s = stream ? (hipStream_t)stream : c->stream;
	HIPCHK(hipSetDevice(c->device));
	return mosrx_launch_nat_patch(&pp, (void *)s);
}

/* ---- over a batch queue (mosrx_queue_set_nat) -------------------------------------- */

int mosrx__nat_queue_check(const mosrx_ctx *c, const mosrx_queue *q)
{
	if (!q->fwd || q->acl || c->params.skip_tcp_csum)
		return -EINVAL;
	return c->d_nat ? 0 : -ENOENT;
}

int mosrx__nat_queue_launch_plan(mosrx_ctx *c, const mosrx_queue *q, void *stream)
{
	mosrx_nparams np;
	const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	int rc;
	nat_ctx_params(c, &np);
	np.f.rec_bytes = q->compact ? 8u : 16u;
	np.fdesc = q->d_fdesc;
	np.xtab = (mosrx_nat_xlat *const *)q->d_nxtab;
	np.nb = q->nb;
	np.total_tiles = q->fwd_tiles;
	HIPCHK(hipSetDevice(c->device));
	nat_mark_used(c);
	rc = mosrx_launch_nat_plan(&np, (void *)s);
	mosrx__note_stream(c, s);
	return rc;
}

int mosrx__nat_queue_launch_patch(mosrx_ctx *c, const mosrx_queue *q, void *stream)
{
	mosrx_npatch pp;
	const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	int rc;
	memset(&pp, 0, sizeof(pp));
	pp.fdesc = q->d_fdesc;
	pp.xtab = (mosrx_nat_xlat *const *)q->d_nxtab;
	pp.nb = q->nb;
	pp.total_tiles = q->fwd_tiles;
	pp.nrings = q->fwd_nrings;
	HIPCHK(hipSetDevice(c->device));
	rc = mosrx_launch_nat_patch(&pp, (void *)s);
	mosrx__note_stream(c, s);   /* (it reads the queue's tables: set_nat's drain waits for it) */
	return rc;
}

int mosrx_queue_set_nat(mosrx_ctx *c, mosrx_queue *q, mosrx_nat_xlat *const *d_xlat)
{
	mosrx_nat_xlat **h;
	uint32_t i;
	int rc;
	if (!c || !q)
		return -EINVAL;
	if (!d_xlat) {
		q->nat = 0;
		return 0;
	}
	if (!q->fwd || q->acl)
		return -EINVAL;
	for (i = 0; i < q->nb; i++)
		if (q->h_desc[i].n && !aligned(d_xlat[i], 16))
			return -EINVAL;
	if (!(h = calloc(q->nb, sizeof(*h))))
		return -ENOMEM;
	for (i = 0; i < q->nb; i++)
		h[i] = q->h_desc[i].n ? d_xlat[i] : NULL;
	/* from here a failure leaves the queue without the attachment */
	q->nat = 0;
	rc = hipSetDevice(c->device) == hipSuccess ? 0 : -EIO;
	if (!rc && !q->d_nxtab && hipMalloc((void **)&q->d_nxtab, (size_t)q->nb * sizeof(*h)) != hipSuccess)
		rc = -ENOMEM;
	/* (a run of this queue submitted earlier may still read the table) */
	if (!rc)
		rc = mosrx__drain(c);
	if (!rc && hipMemcpy(q->d_nxtab, h, (size_t)q->nb * sizeof(*h), hipMemcpyHostToDevice) != hipSuccess)
		rc = -EIO;
	free(h);
	if (rc)
		return rc;
	q->nat = 1;
	return 0;
}
