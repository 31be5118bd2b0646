/*
 * hub.c — one steering backend, one io_module endpoint per mTCP core.
 *
 * The backend (opened with cfg.steer = 2 or 3) exposes one batch at a time,
 * sorted and gathered by queue on the GPU (MOSRX_PKT_RX_QUEUE: queue q's
 * records, offsets, lengths and original indices as contiguous runs; with
 * cfg.steer = 3 also MOSRX_PKT_RX_QUEUE_SIDE: its flow hashes, match masks and
 * pkt_info).  The hub hands
 * queue q's run to core q's recv_pkts, the ring an RSS NIC would have filled
 * for that core (core.c:1369-1466 runs one mTCP thread per core, each calling
 * its own recv_pkts).
 *
 * Two rules (mosrx_io_module.h):
 *   - only the owner (core 0's endpoint, on the opening thread) calls the
 *     backend;
 *   - the backend's recv_pkts, which takes the lent batch back, is called only
 *     when every core has moved past its share of the current one.
 *
 * Per netdev the owner publishes a batch by writing the cores' shares, storing
 * the countdown (ncores) and then bumping the epoch with release order.  A
 * core that loads a new epoch (acquire) reads its share; its next recv_pkts
 * decrements the countdown (release).  The owner reads the countdown with
 * acquire order, so at zero every core's reads of the batch happened before
 * the backend call that recycles it.  Every core sees every epoch exactly
 * once, because the epoch cannot move while the core is still counted.
 * Nothing waits: "no new epoch" and "countdown above zero" are idle rounds.
 */
#include <errno.h>
#include <pthread.h>
#include <stdatomic.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mosrx_io_module.h"

#define HUB_MAGIC 0x6D6F736875623031ull   /* "moshub01" */

/* A core's share of the published batch of one netdev: written by the owner
 * before the epoch's release store, read by that core after its acquire load. */
struct hub_share {
	mosrx_queue_view v;
	mosrx_queue_side side;       /* all NULL: the backend gathers no side arrays, or the batch has none */
	mosrx_rx_state state;
	int has_state;
};

/* What one core keeps per netdev; touched by that core's thread only. */
struct hub_core_if {
	uint32_t seen;               /* the last epoch this core took */
	int holding;                 /* it took a share and has not moved past it */
	const struct hub_share *cur; /* that share (NULL: none) */
};

struct hub_if {
	_Alignas(64) _Atomic uint32_t epoch;       /* batches published; 0: none yet */
	_Alignas(64) _Atomic uint32_t remaining;   /* cores that have not moved past the current batch */
	struct hub_share *share;                   /* ncores */
};

struct hub_endpoint {
	uint64_t magic;
	struct mosrx_hub *hub;
	uint32_t core;
	_Alignas(64) struct hub_core_if cif[MOSRX_MAX_DEVICES];
};

struct mosrx_hub {
	const io_module_func *be;
	struct mtcp_thread_context *be_ctx;
	int nif;
	uint32_t ncores;
	pthread_t owner;
	int side;                    /* every netdev of the backend answers MOSRX_PKT_RX_QUEUE_SIDE (cfg.steer = 3) */
	struct hub_if *ifs;          /* nif */
	struct hub_endpoint *ep;     /* ncores */
	mosrx_hub_stats stats;       /* the owner's */
};

static struct hub_endpoint *ep_of(struct mtcp_thread_context *ctx, int ifidx)
{
	struct hub_endpoint *e = (struct hub_endpoint *)ctx;
	if (!e || e->magic != HUB_MAGIC || !e->hub || ifidx < 0 || ifidx >= e->hub->nif)
		return NULL;
	return e;
}

/* The owner, with every core past the current batch: the backend's next batch
 * (which takes the current one back), published to the cores. */
static int32_t hub_pump(struct mosrx_hub *h, int ifidx)
{
	struct hub_if *hi = &h->ifs[ifidx];
	mosrx_rx_state state;
	uint64_t sum = 0;
	uint32_t q;
	int has_state;
	const int32_t n = h->be->recv_pkts(h->be_ctx, ifidx);
	if (n <= 0)
		return n;
	memset(&state, 0, sizeof(state));
	has_state = h->be->dev_ioctl(h->be_ctx, ifidx, MOSRX_PKT_RX_STATE, &state) == 0;
	for (q = 0; q < h->ncores; q++) {
		struct hub_share *s = &hi->share[q];
		memset(s, 0, sizeof(*s));
		s->v.q = q;
		if (h->be->dev_ioctl(h->be_ctx, ifidx, MOSRX_PKT_RX_QUEUE, &s->v) || s->v.n > (uint32_t)n ||
		    (s->v.n && (!s->v.rec || !s->v.off || !s->v.len || !s->v.idx || !s->v.frames)))
			return -1;   /* not a gathered batch: nothing is published, the next call moves on */
		/* its side arrays: on this thread too; a batch gathered without them leaves the share's pointers NULL */
		s->side.q = q;
		if (!h->side || h->be->dev_ioctl(h->be_ctx, ifidx, MOSRX_PKT_RX_QUEUE_SIDE, &s->side) || s->side.n != s->v.n)
			memset(&s->side, 0, sizeof(s->side));
		s->side.q = q;
		s->side.n = s->v.n;
		s->state = state;
		s->state.n = s->v.n;
		s->state.rec_bytes = s->v.rec_bytes;
		s->has_state = has_state;
		sum += s->v.n;
	}
	if (sum > (uint64_t)n)
		return -1;
	h->stats.batches++;
	h->stats.frames += (uint64_t)n;
	h->stats.delivered += sum;
	h->stats.unowned += (uint64_t)n - sum;
	atomic_store_explicit(&hi->remaining, h->ncores, memory_order_relaxed);
	atomic_fetch_add_explicit(&hi->epoch, 1, memory_order_release);
	return n;
}

static int32_t hub_recv_pkts(struct mtcp_thread_context *ctx, int ifidx)
{
	struct hub_endpoint *e = ep_of(ctx, ifidx);
	struct mosrx_hub *h;
	struct hub_if *hi;
	struct hub_core_if *c;
	uint32_t ep;
	if (!e)
		return -1;
	h = e->hub;
	hi = &h->ifs[ifidx];
	c = &e->cif[ifidx];
	if (e->core == 0 && !pthread_equal(pthread_self(), h->owner))
		return -1;
	if (c->holding) {            /* this call moves the core past its share */
		c->holding = 0;
		c->cur = NULL;
		atomic_fetch_sub_explicit(&hi->remaining, 1, memory_order_release);
	}
	if (e->core == 0) {
		int32_t n;
		if (atomic_load_explicit(&hi->remaining, memory_order_acquire) != 0) {
			h->stats.owner_waits++;
			return 0;
		}
		if ((n = hub_pump(h, ifidx)) <= 0)
			return n;
	}
	ep = atomic_load_explicit(&hi->epoch, memory_order_acquire);
	if (ep == c->seen)
		return 0;
	c->seen = ep;
	c->cur = &hi->share[e->core];
	if (c->cur->v.n == 0) {      /* an empty share: counted once, now */
		c->cur = NULL;
		atomic_fetch_sub_explicit(&hi->remaining, 1, memory_order_release);
		return 0;
	}
	c->holding = 1;
	return (int32_t)c->cur->v.n;
}

static uint8_t *hub_get_rptr(struct mtcp_thread_context *ctx, int ifidx, int index, uint16_t *len)
{
	struct hub_endpoint *e = ep_of(ctx, ifidx);
	const struct hub_share *s = e ? e->cif[ifidx].cur : NULL;
	if (!s || index < 0 || (uint32_t)index >= s->v.n)
		return NULL;
	*len = s->v.len[index];
	return (uint8_t *)(uintptr_t)(s->v.frames + s->v.off[index]);
}

static int32_t hub_send_pkts(struct mtcp_thread_context *ctx, int nif)
{
	struct hub_endpoint *e = ep_of(ctx, nif);
	if (!e)
		return -1;
	/* the round's TX flush is the backend's, so the owner's */
	if (e->core == 0 && e->hub->be->send_pkts && pthread_equal(pthread_self(), e->hub->owner))
		return e->hub->be->send_pkts(e->hub->be_ctx, nif);
	return 0;
}

static int32_t hub_dev_ioctl(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp)
{
	struct hub_endpoint *e = ep_of(ctx, nif);
	const struct hub_share *s = e ? e->cif[nif].cur : NULL;
	if (!s || !argp)
		return -1;
	switch (cmd) {
	case PKT_RX_RSS: {
		RssInfo *ri = argp;
		const uint8_t *r;
		if (ri->pktidx < 0 || (uint32_t)ri->pktidx >= s->v.n)
			return -1;
		r = s->v.rec + (size_t)ri->pktidx * s->v.rec_bytes;
		ri->hash_value = s->v.rec_bytes == sizeof(mosrx_result8) ? ((const mosrx_result8 *)r)->rss
		                                                         : ((const mosrx_result *)r)->rss;
		return 0;
	}
	case MOSRX_PKT_RX_RESULTS:
		if (s->v.rec_bytes != sizeof(mosrx_result))
			return -1;
		*(const mosrx_result **)argp = (const mosrx_result *)s->v.rec;
		return 0;
	case MOSRX_PKT_RX_RESULTS8:
		if (s->v.rec_bytes != sizeof(mosrx_result8))
			return -1;
		*(const mosrx_result8 **)argp = (const mosrx_result8 *)s->v.rec;
		return 0;
	case MOSRX_PKT_RX_STATE:
		if (!s->has_state)
			return -1;
		*(mosrx_rx_state *)argp = s->state;
		return 0;
	case MOSRX_PKT_RX_QUEUE:     /* the share's own view, whatever q asks */
		*(mosrx_queue_view *)argp = s->v;
		return 0;
	/* the share's runs of the batch's side arrays (frame i of the share at [i], as get_rptr(i)) */
	case MOSRX_PKT_RX_MATCH:
		if (!s->side.match)
			return -1;
		*(const uint32_t **)argp = s->side.match;
		return 0;
	case MOSRX_PKT_RX_FHASH:
		if (!s->side.fhash)
			return -1;
		*(const uint32_t **)argp = s->side.fhash;
		return 0;
	case MOSRX_PKT_RX_TCPINFO:
		if (!s->side.tcpinfo)
			return -1;
		*(const mosrx_tcpinfo **)argp = s->side.tcpinfo;
		return 0;
	case MOSRX_PKT_RX_QUEUE_SIDE:
		if (!e->hub->side)
			return -1;
		*(mosrx_queue_side *)argp = s->side;
		return 0;
	case MOSRX_PKT_RX_FWD:       /* forwarding behind the hub is not built: an endpoint has no view */
		return -1;
	default:
		return -1;
	}
}

io_module_func mosrx_hub_module_func = {
	.send_pkts = hub_send_pkts,
	.get_rptr = hub_get_rptr,
	.recv_pkts = hub_recv_pkts,
	.dev_ioctl = hub_dev_ioctl,
};

int mosrx_hub_open(const io_module_func *backend, struct mtcp_thread_context *backend_ctx, int nif,
                   uint32_t ncores, mosrx_hub **out)
{
	struct mosrx_hub *h;
	mosrx_queue_view probe;
	mosrx_queue_side sprobe;
	uint32_t q;
	int i, side = 1;
	if (out)
		*out = NULL;
	if (!backend || !backend->recv_pkts || !out || nif <= 0 || nif > MOSRX_MAX_DEVICES || ncores == 0 ||
	    ncores > MOSRX_HUB_MAX_CORES)
		return -EINVAL;
	if (!backend->dev_ioctl)
		return -ENOTSUP;
	for (i = 0; i < nif; i++) {
		memset(&probe, 0, sizeof(probe));
		probe.q = MOSRX_QUEUE_PROBE;
		if (backend->dev_ioctl(backend_ctx, i, MOSRX_PKT_RX_QUEUE, &probe))
			return -ENOTSUP;
		memset(&sprobe, 0, sizeof(sprobe));
		sprobe.q = MOSRX_QUEUE_PROBE;
		if (backend->dev_ioctl(backend_ctx, i, MOSRX_PKT_RX_QUEUE_SIDE, &sprobe))
			side = 0;   /* a cfg.steer = 2 backend: records and descriptors only, as before */
	}
	if (!(h = calloc(1, sizeof(*h))))
		return -ENOMEM;
	h->be = backend;
	h->be_ctx = backend_ctx;
	h->nif = nif;
	h->ncores = ncores;
	h->owner = pthread_self();
	h->side = side;
	if (posix_memalign((void **)&h->ifs, 64, (size_t)nif * sizeof(*h->ifs)))
		h->ifs = NULL;
	if (posix_memalign((void **)&h->ep, 64, (size_t)ncores * sizeof(*h->ep)))
		h->ep = NULL;
	if (!h->ifs || !h->ep) {
		free(h->ifs);
		free(h->ep);
		free(h);
		return -ENOMEM;
	}
	memset(h->ifs, 0, (size_t)nif * sizeof(*h->ifs));
	memset(h->ep, 0, (size_t)ncores * sizeof(*h->ep));
	for (i = 0; i < nif; i++) {
		atomic_init(&h->ifs[i].epoch, 0);
		atomic_init(&h->ifs[i].remaining, 0);
		if (!(h->ifs[i].share = calloc(ncores, sizeof(*h->ifs[i].share)))) {
			while (i-- > 0)
				free(h->ifs[i].share);
			free(h->ifs);
			free(h->ep);
			free(h);
			return -ENOMEM;
		}
	}
	for (q = 0; q < ncores; q++) {
		h->ep[q].magic = HUB_MAGIC;
		h->ep[q].hub = h;
		h->ep[q].core = q;
	}
	*out = h;
	return 0;
}

struct mtcp_thread_context *mosrx_hub_endpoint(mosrx_hub *hub, uint32_t core)
{
	if (!hub || core >= hub->ncores)
		return NULL;
	return (struct mtcp_thread_context *)&hub->ep[core];
}

int mosrx_hub_stats_get(const mosrx_hub *hub, mosrx_hub_stats *st)
{
	if (!hub || !st)
		return -EINVAL;
	*st = hub->stats;
	return 0;
}

int mosrx_hub_close(mosrx_hub *hub)
{
	uint32_t q;
	int i;
	if (!hub)
		return -EINVAL;
	for (i = 0; i < hub->nif; i++)
		if (atomic_load_explicit(&hub->ifs[i].remaining, memory_order_acquire) != 0)
			return -EBUSY;
	for (q = 0; q < hub->ncores; q++)
		hub->ep[q].magic = 0;
	for (i = 0; i < hub->nif; i++)
		free(hub->ifs[i].share);
	free(hub->ifs);
	free(hub->ep);
	free(hub);
	return 0;
}
