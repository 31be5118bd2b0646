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

/* ---- the table (its arithmetic: nat_table.c) ---------------------------------------- */

uint32_t mosrx_nat_count(const mosrx_ctx *c) { return c ? c->nat_n : 0; }

int mosrx_nat_get_stats(const mosrx_ctx *c, mosrx_nat_stats *out)
{
	if (!c || !out)
		return -EINVAL;
	memset(out, 0, sizeof(*out));
	out->live = c->nat_n;
	out->tombs = c->nat_st.tombs;
	out->slots = c->d_nat ? c->nat_mask + 1 : 0;
	out->probe = c->nat_probe;
	out->updates = c->nat_updates;
	out->rebuilds = c->nat_rebuilds;
	return 0;
}

/* The host table h (cap slots, n bindings, no tombstones; the context's from
 * here on success) goes to the next buffer of a pool, as the forwarding tables
 * do (fwd_api.c mosrx_fwd_set): launches submitted earlier may still read or
 * update the copy they were given, so a buffer is written again (or freed to
 * grow) only after those launches drained, and only if a launch may have touched
 * it since its last write. */
static int nat_install(mosrx_ctx *c, mosrx_nat_slot *h, uint32_t cap, uint32_t n, uint32_t probe)
{
	const size_t bytes = (size_t)cap * sizeof(*h);
	const uint32_t k = c->nat_pool_next;
	int rc = 0;
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
	if (rc)
		return rc;
	c->d_nat = c->d_nat_pool[k];
	c->nat_n = n;
	c->nat_mask = cap - 1;
	c->nat_probe = probe;
	c->nat_pool_next = (k + 1) % MOSRX_NAT_POOL;
	free(c->nat_h);
	c->nat_h = h;
	c->nat_st.slots = cap;
	c->nat_st.keys = 2 * n;
	c->nat_st.tombs = 0;
	c->nat_st.probe = probe;
	return 0;
}

int mosrx_nat_set(mosrx_ctx *c, const mosrx_nat_binding *b, uint32_t n)
{
	mosrx_nat_slot *h;
	uint32_t probe = 0, cap;
	int rc;
	if (!c || n > MOSRX_NAT_MAX_BINDINGS || (n && !b))
		return -EINVAL;
	if (!b)
		n = 0;
	cap = mosrx_nat_slots(n);
	if (!(h = malloc((size_t)cap * sizeof(*h))))
		return -ENOMEM;
	if ((rc = mosrx_nat_build(b, n, h, &probe)) || (rc = nat_install(c, h, cap, n, probe)))
		free(h);
	return rc;
}

void mosrx__nat_free(mosrx_ctx *c)
{
	uint32_t i;
	for (i = 0; i < MOSRX_NAT_POOL; i++)
		if (c->d_nat_pool[i])
			hipFree(c->d_nat_pool[i]);
	for (i = 0; i < MOSRX_NAT_STAGE; i++) {
		if (c->nat_stage[i].busy)
			hipEventSynchronize(c->nat_stage[i].ev);
		if (c->nat_stage[i].ev)
			hipEventDestroy(c->nat_stage[i].ev);
		if (c->nat_stage[i].h)
			hipHostFree(c->nat_stage[i].h);
	}
	for (i = 0; i < MOSRX_NAT_OWN; i++)
		if (c->nat_own_ev[i])
			hipEventDestroy(c->nat_own_ev[i]);
	free(c->nat_h);
}

/* The context's own stream number k (mosrx_ctx.h nat_own_mask), NULL past the last. */
static hipStream_t nat_own_stream(const mosrx_ctx *c, uint32_t k)
{
	if (k == 0)
		return c->stream;
	if (k < 1 + NSLOT)
		return c->slot[k - 1].stream;
	return k - 1 - NSLOT < c->nxs ? c->xs[k - 1 - NSLOT] : NULL;
}

/* A launch that reads the installed table is about to go to stream s. */
static void nat_mark_used(mosrx_ctx *c, hipStream_t s)
{
	uint32_t k;
	c->nat_pool_used[(c->nat_pool_next + MOSRX_NAT_POOL - 1) % MOSRX_NAT_POOL] = 1;
	mosrx__fwd_mark_used(c);
	/* (a caller's stream: mosrx__note_stream records its event behind the launch) */
	for (k = 0; k < MOSRX_NAT_OWN; k++)
		if (s && s == nat_own_stream(c, k))
			c->nat_own_mask |= 1u << k;
}

/* ---- bindings added and removed in place ------------------------------------------- */

/* Stream s waits, on the device, for what an update must not overtake: the
 * plan-nat launches made on other streams and the update before this one.  The
 * callers' streams' events are those mosrx__note_stream recorded behind each
 * launch; on the context's own streams an event is recorded now.  More callers'
 * streams than the table holds: the host drains instead. */
static int nat_order(mosrx_ctx *c, hipStream_t s)
{
	const uint32_t last = (c->nat_stage_next + MOSRX_NAT_STAGE - 1) % MOSRX_NAT_STAGE;
	uint32_t k;
	if (c->foreign_streams)
		return mosrx__drain(c);
	for (k = 0; k < c->nfs; k++)
		if (c->fstream[k] != s)
			HIPCHK(hipStreamWaitEvent(s, c->fev[k], 0));
	for (k = 0; k < MOSRX_NAT_OWN; k++) {
		const hipStream_t t = nat_own_stream(c, k);
		if (!(c->nat_own_mask & 1u << k) || !t || t == s)
			continue;
		if (!c->nat_own_ev[k])
			HIPCHK(hipEventCreateWithFlags(&c->nat_own_ev[k], hipEventDisableTiming));
		HIPCHK(hipEventRecord(c->nat_own_ev[k], t));
		HIPCHK(hipStreamWaitEvent(s, c->nat_own_ev[k], 0));
	}
	if (c->nat_stage[last].busy && c->nat_stage[last].stream != s)
		HIPCHK(hipStreamWaitEvent(s, c->nat_stage[last].ev, 0));
	return 0;
}

/* The staging buffer of the next update with room for `need` entries, free of
 * the launch that read it last. */
static int nat_stage_take(mosrx_ctx *c, uint32_t need, uint32_t *which)
{
	const uint32_t k = c->nat_stage_next;
	if (c->nat_stage[k].busy) {
		HIPCHK(hipEventSynchronize(c->nat_stage[k].ev));
		c->nat_stage[k].busy = 0;
	}
	if (!c->nat_stage[k].ev)
		HIPCHK(hipEventCreateWithFlags(&c->nat_stage[k].ev, hipEventDisableTiming));
	if (c->nat_stage[k].cap < need) {
		void *d = NULL;
		uint32_t cap = 256;
		while (cap < need)
			cap <<= 1;
		if (c->nat_stage[k].h)
			hipHostFree(c->nat_stage[k].h);
		c->nat_stage[k].h = NULL;
		c->nat_stage[k].cap = 0;
		if (hipHostMalloc((void **)&c->nat_stage[k].h, (size_t)cap * sizeof(mosrx_nat_touch), hipHostMallocDefault) != hipSuccess)
			return -ENOMEM;
		if (hipHostGetDevicePointer(&d, c->nat_stage[k].h, 0) != hipSuccess)
			return -EIO;   /* (cap stays 0: the next call allocates again) */
		c->nat_stage[k].d = (const mosrx_nat_touch *)d;
		c->nat_stage[k].cap = cap;
	}
	*which = k;
	return 0;
}

/* The table is too full of keys and tombstones for the ops: the live bindings
 * and the ops into a fresh one.  The ops run, by mosrx_nat_apply and so under
 * its refusals, on a scratch table with room for all of them; what is live
 * there is then built without tombstones and installed.  Nothing of the context
 * changes before the install. */
static int nat_rebuild(mosrx_ctx *c, const mosrx_nat_op *ops, uint32_t n)
{
	const uint32_t live = c->nat_st.keys / 2;
	uint32_t cap = MOSRX_NAT_MIN_SLOTS, m = 0, left, probe = 0, *ids = NULL;
	mosrx_nat_binding *b = NULL;
	mosrx_nat_slot *h = NULL, *scratch = NULL;
	mosrx_nat_touch *touch = NULL;
	mosrx_nat_tstate st;
	int rc = -ENOMEM;
	while (cap < 4u * (live + n))
		cap <<= 1;
	b = malloc(((size_t)live + n + 1) * sizeof(*b));
	ids = malloc(((size_t)live + n + 1) * sizeof(*ids));
	scratch = malloc((size_t)cap * sizeof(*scratch));
	touch = malloc((size_t)4 * n * sizeof(*touch));
	if (!b || !ids || !scratch || !touch)
		goto out;
	/* the live keys as they lie, without the tombstones, into the scratch table */
	mosrx__nat_live(c->nat_h, c->nat_st.slots, b, ids, live);
	if ((rc = mosrx__nat_build_ids(b, ids, live, scratch, cap, &probe)))
		goto out;   /* (the mirror's own keys collide: not a table of ours) */
	st.slots = cap;
	st.keys = 2 * live;
	st.tombs = 0;
	st.probe = probe;
	if ((rc = mosrx_nat_apply(scratch, &st, ops, n, touch, &m)))
		goto out;
	left = mosrx__nat_live(scratch, cap, b, ids, live + n);
	rc = -ENOMEM;
	if (!(h = malloc((size_t)mosrx_nat_slots(left) * sizeof(*h))))
		goto out;
	if ((rc = mosrx__nat_build_ids(b, ids, left, h, 0, &probe)) || (rc = nat_install(c, h, mosrx_nat_slots(left), left, probe)))
		free(h);
out:
	free(b);
	free(ids);
	free(scratch);
	free(touch);
	return rc;
}

int mosrx_nat_update(mosrx_ctx *c, const mosrx_nat_op *ops, uint32_t n, void *stream)
{
	mosrx_nat_tstate st;
	hipStream_t s;
	uint32_t k, m = 0;
	int rc;
	if (!c || (n && !ops) || n > MOSRX_NAT_UPDATE_MAX_OPS)
		return -EINVAL;
	if (n == 0)
		return 0;
	HIPCHK(hipSetDevice(c->device));
	if (!c->d_nat) {
		/* never set: the empty table, installed once every op is known to be acceptable to it -- tried on a
		 * scratch table with room for all of them (each op adds at most two keys or tombstones) */
		uint32_t cap = MOSRX_NAT_MIN_SLOTS;
		mosrx_nat_slot *scratch;
		mosrx_nat_touch *t;
		while (cap < 4u * n)
			cap <<= 1;
		scratch = calloc(cap, sizeof(*scratch));
		t = malloc((size_t)4 * n * sizeof(*t));
		rc = -ENOMEM;
		if (scratch && t) {
			st.slots = cap;
			st.keys = st.tombs = st.probe = 0;
			rc = mosrx_nat_apply(scratch, &st, ops, n, t, &m);
		}
		free(scratch);
		free(t);
		if (rc || (rc = mosrx_nat_set(c, NULL, 0)))
			return rc;
	}
	s = stream ? (hipStream_t)stream : c->stream;
	/* what can fail in the runtime comes before the mirror changes: the staging buffer, the waits */
	if ((rc = nat_stage_take(c, 4u * n, &k)) || (rc = nat_order(c, s)))
		return rc;
	st = c->nat_st;
	rc = mosrx_nat_apply(c->nat_h, &st, ops, n, c->nat_stage[k].h, &m);
	if (rc == -ENOSPC) {
		if (!(rc = nat_rebuild(c, ops, n))) {
			c->nat_updates++;
			c->nat_rebuilds++;
		}
		return rc;
	}
	if (rc)
		return rc;
	/* The mirror has changed.  Should the launch itself fail (-EIO: the runtime's) the device copy stays
	 * behind it; mosrx_nat_set installs a whole table again. */
	c->nat_st = st;
	c->nat_n = st.keys / 2;
	c->nat_probe = st.probe;
	c->nat_pool_used[(c->nat_pool_next + MOSRX_NAT_POOL - 1) % MOSRX_NAT_POOL] = 1;
	if ((rc = mosrx_launch_nat_update(c->d_nat, c->nat_mask, c->nat_stage[k].d, m, (void *)s)))
		return rc;
	c->nat_updates++;
	c->nat_own_mask = 0;
	mosrx__note_stream(c, s);   /* (a caller's stream: the drain ahead of this copy's next rewrite waits for it) */
	if (hipEventRecord(c->nat_stage[k].ev, s) != hipSuccess) {
		/* no event to tell when the launch has read the buffer: wait for it here */
		HIPCHK(hipStreamSynchronize(s));
		return 0;
	}
	c->nat_stage[k].busy = 1;
	c->nat_stage[k].stream = s;
	c->nat_stage_next = (k + 1) % MOSRX_NAT_STAGE;
	return 0;
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
	nat_mark_used(c, s);
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
	nat_mark_used(c, s);
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
