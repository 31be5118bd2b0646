/*
 * hub_stub.c — a stand-in steering + gathering io_module_func for the hub's
 * CPU tests (tests/test_hub.py, tests/csrc/hub_driver.c): it exposes the
 * batches the test set, one per recv_pkts, already sorted queue-major (by
 * numpy / the driver), serves MOSRX_PKT_RX_QUEUE views over them, and records
 * every backend call with the calling thread and the number of frames the
 * cores' consumers had taken by then -- a recv_pkts that arrives before every
 * core walked its share of the batch it takes back shows in that number.
 */
#include <pthread.h>
#include <stdatomic.h>
#include <stddef.h>
#include <string.h>
#include <unistd.h>

#include "mosrx_io_module.h"

typedef struct hub_stub_batch {
	const uint8_t *frames;
	const uint8_t *qrec;        /* n records of rec_bytes, queue-major */
	const uint32_t *qoff;
	const uint16_t *qlen;
	const uint32_t *idx;
	const uint32_t *qstart;     /* MOSRX_STEER_QSLOTS */
	uint32_t n;
	uint32_t rec_bytes;
} hub_stub_batch;

enum { HUB_CALL_RECV = 1, HUB_CALL_IOCTL = 2, HUB_CALL_SEND = 3, HUB_CALL_RPTR = 4 };

typedef struct hub_stub_call {
	uint64_t tid;
	uint64_t consumed;          /* frames the consumers had taken when the call arrived */
	uint32_t what;              /* HUB_CALL_* */
	int32_t cur;                /* the batch exposed when it arrived, -1 none */
} hub_stub_call;

/* One core's consumer state: the argument of hub_stub_consume. */
typedef struct hub_stub_delivery {
	uint32_t batch, orig;       /* the backend's batch, the frame's index in it (the endpoint's idx) */
	int32_t index;              /* its index in the share */
	uint32_t len, sum;          /* frame length and byte sum */
	uint8_t rec[16];            /* the record handed over (16-byte form) */
} hub_stub_delivery;

typedef struct hub_stub_core {
	struct mtcp_thread_context *ep;
	int32_t (*dev_ioctl)(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp);
	hub_stub_delivery *log;
	uint32_t log_cap, log_n;
	uint32_t sleep_us, sleep_every;   /* a deliberately slow core: sleep_us every sleep_every frames */
	uint32_t bad;                     /* deliveries whose view did not answer */
} hub_stub_core;

static const hub_stub_batch *g_b;
static uint32_t g_nb, g_next, g_gather;
static int g_cur = -1;
static hub_stub_call *g_calls;
static uint32_t g_calls_cap;
static _Atomic uint32_t g_calls_n;
static _Atomic uint64_t g_consumed;
static _Atomic uint32_t g_exhausted;

void hub_stub_set(const hub_stub_batch *b, uint32_t nb, int gather, hub_stub_call *calls, uint32_t calls_cap)
{
	g_b = b;
	g_nb = nb;
	g_next = 0;
	g_cur = -1;
	g_gather = (uint32_t)gather;
	g_calls = calls;
	g_calls_cap = calls_cap;
	atomic_store(&g_calls_n, 0);
	atomic_store(&g_consumed, 0);
	atomic_store(&g_exhausted, 0);
}

uint32_t hub_stub_calls(void) { return atomic_load(&g_calls_n); }
uint32_t hub_stub_exhausted(void) { return atomic_load(&g_exhausted); }
uint64_t hub_stub_consumed(void) { return atomic_load(&g_consumed); }
uint64_t hub_stub_self(void) { return (uint64_t)(uintptr_t)pthread_self(); }

static void note(uint32_t what)
{
	const uint32_t k = atomic_fetch_add(&g_calls_n, 1);
	if (g_calls && k < g_calls_cap) {
		g_calls[k].tid = hub_stub_self();
		g_calls[k].consumed = atomic_load(&g_consumed);
		g_calls[k].what = what;
		g_calls[k].cur = g_cur;
	}
}

static int32_t stub_recv_pkts(struct mtcp_thread_context *ctx, int ifidx)
{
	(void)ctx;
	note(HUB_CALL_RECV);
	if (ifidx != 0)
		return -1;
	if (g_next >= g_nb) {
		g_cur = -1;
		atomic_store(&g_exhausted, 1);
		return 0;
	}
	g_cur = (int)g_next++;
	return (int32_t)g_b[g_cur].n;
}

static uint8_t *stub_get_rptr(struct mtcp_thread_context *ctx, int ifidx, int index, uint16_t *len)
{
	(void)ctx;
	(void)ifidx;
	(void)index;
	(void)len;
	note(HUB_CALL_RPTR);         /* the hub reads frames through the views, never through the backend */
	return NULL;
}

static int32_t stub_send_pkts(struct mtcp_thread_context *ctx, int nif)
{
	(void)ctx;
	(void)nif;
	note(HUB_CALL_SEND);
	return 0;
}

static int32_t stub_dev_ioctl(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp)
{
	const hub_stub_batch *b;
	(void)ctx;
	note(HUB_CALL_IOCTL);
	if (nif != 0 || !argp)
		return -1;
	if (cmd == MOSRX_PKT_RX_QUEUE && ((mosrx_queue_view *)argp)->q == MOSRX_QUEUE_PROBE)
		return g_gather ? 0 : -1;
	if (g_cur < 0)
		return -1;
	b = &g_b[g_cur];
	switch (cmd) {
	case MOSRX_PKT_RX_STATE: {
		mosrx_rx_state *s = argp;
		memset(s, 0, sizeof(*s));
		s->gen = 7;
		s->n = b->n;
		s->rec_bytes = b->rec_bytes;
		return 0;
	}
	case MOSRX_PKT_RX_QUEUE: {
		mosrx_queue_view *v = argp;
		uint32_t q0;
		if (!g_gather || v->q >= MOSRX_STEER_QSLOTS - 1)
			return -1;
		q0 = b->qstart[v->q];
		v->n = b->qstart[v->q + 1] - q0;
		v->rec_bytes = b->rec_bytes;
		v->rec = b->qrec + (size_t)q0 * b->rec_bytes;
		v->off = b->qoff + q0;
		v->len = b->qlen + q0;
		v->idx = b->idx + q0;
		v->frames = b->frames;
		return 0;
	}
	default:
		return -1;
	}
}

/* mosrx_pkt_fn of one core: arg is its hub_stub_core. */
void hub_stub_consume(void *arg, int ifidx, int index, const uint8_t *pkt, uint16_t len, const mosrx_result *res)
{
	hub_stub_core *c = arg;
	mosrx_queue_view v;
	mosrx_rx_state st;
	uint32_t sum = 0, j;
	memset(&v, 0, sizeof(v));
	memset(&st, 0, sizeof(st));
	if (c->dev_ioctl(c->ep, ifidx, MOSRX_PKT_RX_QUEUE, &v) || (uint32_t)index >= v.n ||
	    c->dev_ioctl(c->ep, ifidx, MOSRX_PKT_RX_STATE, &st) || st.n != v.n || st.gen != 7)
		c->bad++;
	for (j = 0; j < len; j++)
		sum += pkt[j];
	if (c->log && c->log_n < c->log_cap) {
		hub_stub_delivery *d = &c->log[c->log_n];
		/* the exposed batch cannot change while this core holds a share of it */
		d->batch = (uint32_t)g_cur;
		d->orig = (uint32_t)index < v.n ? v.idx[index] : 0xFFFFFFFFu;
		d->index = index;
		d->len = len;
		d->sum = sum;
		memcpy(d->rec, res, sizeof(d->rec));
	}
	c->log_n++;
	atomic_fetch_add(&g_consumed, 1);
	if (c->sleep_us && c->sleep_every && c->log_n % c->sleep_every == 0)
		usleep(c->sleep_us);
}

io_module_func hub_stub_func = {
	.send_pkts = stub_send_pkts,
	.get_rptr = stub_get_rptr,
	.recv_pkts = stub_recv_pkts,
	.dev_ioctl = stub_dev_ioctl,
};
