/*
 * hub_side_stub.c — hub_stub.c's stand-in backend plus the side arrays, for
 * tests/test_hub_side.py and tests/csrc/hub_side_driver.c: it exposes the
 * batches the test set, one per recv_pkts, already sorted queue-major, serves
 * MOSRX_PKT_RX_QUEUE and (when told to) MOSRX_PKT_RX_QUEUE_SIDE views over
 * them, and records every backend call with its command and calling thread.
 * A core's consumer asks its endpoint for RX_MATCH / RX_FHASH / RX_TCPINFO and
 * logs what it finds at the frame's index in the share.
 */
#include <pthread.h>
#include <stdatomic.h>
#include <stddef.h>
#include <string.h>

#include "mosrx_io_module.h"

typedef struct hub_side_batch {
	const uint8_t *frames;
	const uint8_t *qrec;        /* n records of rec_bytes, queue-major */
	const uint32_t *qoff;
	const uint16_t *qlen;
	const uint32_t *idx;
	const uint32_t *qstart;     /* MOSRX_STEER_QSLOTS */
	const uint32_t *qfhash;     /* queue-major side arrays; NULL: the batch has none */
	const uint32_t *qmatch;
	const mosrx_tcpinfo *qtcpinfo;
	uint32_t n;
	uint32_t rec_bytes;
} hub_side_batch;

typedef struct hub_side_call {
	uint64_t tid;
	uint32_t what;              /* 1 recv_pkts, 2 dev_ioctl, 3 send_pkts, 4 get_rptr */
	int32_t cmd;                /* dev_ioctl's command */
} hub_side_call;

#define HUB_SIDE_NONE 0xFFFFFFFFu
typedef struct hub_side_delivery {
	uint32_t batch, orig;       /* the backend's batch, the frame's index in it */
	int32_t index;              /* its index in the share */
	uint32_t has;               /* bit 0 RX_FHASH answered, 1 RX_MATCH, 2 RX_TCPINFO, 3 RX_QUEUE_SIDE */
	uint32_t fhash, match;      /* [index] of the endpoint's arrays */
	mosrx_tcpinfo ti;
	uint32_t side_n;            /* RX_QUEUE_SIDE's n, and whether its pointers are the three above */
	uint32_t side_same;
} hub_side_delivery;

typedef struct hub_side_core {
	struct mtcp_thread_context *ep;
	int32_t (*dev_ioctl)(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp);
	hub_side_delivery *log;
	uint32_t log_cap, log_n;
	uint32_t bad;               /* deliveries whose view did not answer */
} hub_side_core;

static const hub_side_batch *g_b;
static uint32_t g_nb, g_next, g_side;
static int g_cur = -1;
static hub_side_call *g_calls;
static uint32_t g_calls_cap;
static _Atomic uint32_t g_calls_n;

void hub_side_set(const hub_side_batch *b, uint32_t nb, int side, hub_side_call *calls, uint32_t calls_cap)
{
	g_b = b;
	g_nb = nb;
	g_next = 0;
	g_cur = -1;
	g_side = (uint32_t)side;
	g_calls = calls;
	g_calls_cap = calls_cap;
	atomic_store(&g_calls_n, 0);
}

uint32_t hub_side_calls(void) { return atomic_load(&g_calls_n); }
uint64_t hub_side_self(void) { return (uint64_t)(uintptr_t)pthread_self(); }

static void note(uint32_t what, int cmd)
{
	const uint32_t k = atomic_fetch_add(&g_calls_n, 1);
	if (g_calls && k < g_calls_cap) {
		g_calls[k].tid = hub_side_self();
		g_calls[k].what = what;
		g_calls[k].cmd = cmd;
	}
}

static int32_t stub_recv_pkts(struct mtcp_thread_context *ctx, int ifidx)
{
	(void)ctx;
	note(1, 0);
	if (ifidx != 0)
		return -1;
	if (g_next >= g_nb) {
		g_cur = -1;
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
	note(4, 0);
	return NULL;
}

static int32_t stub_send_pkts(struct mtcp_thread_context *ctx, int nif)
{
	(void)ctx;
	(void)nif;
	note(3, 0);
	return 0;
}

static int32_t stub_dev_ioctl(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp)
{
	const hub_side_batch *b;
	(void)ctx;
	note(2, cmd);
	if (nif != 0 || !argp)
		return -1;
	if (cmd == MOSRX_PKT_RX_QUEUE && ((mosrx_queue_view *)argp)->q == MOSRX_QUEUE_PROBE)
		return 0;
	if (cmd == MOSRX_PKT_RX_QUEUE_SIDE && ((mosrx_queue_side *)argp)->q == MOSRX_QUEUE_PROBE)
		return g_side ? 0 : -1;
	if (g_cur < 0)
		return -1;
	b = &g_b[g_cur];
	switch (cmd) {
	case MOSRX_PKT_RX_QUEUE: {
		mosrx_queue_view *v = argp;
		uint32_t q0;
		if (v->q >= MOSRX_STEER_QSLOTS - 1)
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
	case MOSRX_PKT_RX_QUEUE_SIDE: {
		mosrx_queue_side *v = argp;
		uint32_t q0;
		if (!g_side || v->q >= MOSRX_STEER_QSLOTS - 1)
			return -1;
		q0 = b->qstart[v->q];
		v->n = b->qstart[v->q + 1] - q0;
		v->fhash = b->qfhash ? b->qfhash + q0 : NULL;
		v->match = b->qmatch ? b->qmatch + q0 : NULL;
		v->tcpinfo = b->qtcpinfo ? b->qtcpinfo + q0 : NULL;
		return 0;
	}
	default:
		return -1;
	}
}

/* mosrx_pkt_fn of one core: arg is its hub_side_core. */
void hub_side_consume(void *arg, int ifidx, int index, const uint8_t *pkt, uint16_t len, const mosrx_result *res)
{
	hub_side_core *c = arg;
	mosrx_queue_view v;
	mosrx_queue_side sv;
	const uint32_t *fh = NULL, *mt = NULL;
	const mosrx_tcpinfo *ti = NULL;
	hub_side_delivery d;
	(void)pkt;
	(void)len;
	(void)res;
	memset(&v, 0, sizeof(v));
	memset(&sv, 0, sizeof(sv));
	memset(&d, 0, sizeof(d));
	if (c->dev_ioctl(c->ep, ifidx, MOSRX_PKT_RX_QUEUE, &v) || (uint32_t)index >= v.n) {
		c->bad++;
		c->log_n++;
		return;
	}
	/* the exposed batch cannot change while this core holds a share of it */
	d.batch = (uint32_t)g_cur;
	d.orig = v.idx[index];
	d.index = index;
	d.fhash = d.match = HUB_SIDE_NONE;
	if (c->dev_ioctl(c->ep, ifidx, MOSRX_PKT_RX_FHASH, &fh) == 0 && fh) {
		d.has |= 1u;
		d.fhash = fh[index];
	}
	if (c->dev_ioctl(c->ep, ifidx, MOSRX_PKT_RX_MATCH, &mt) == 0 && mt) {
		d.has |= 2u;
		d.match = mt[index];
	}
	if (c->dev_ioctl(c->ep, ifidx, MOSRX_PKT_RX_TCPINFO, &ti) == 0 && ti) {
		d.has |= 4u;
		d.ti = ti[index];
	}
	if (c->dev_ioctl(c->ep, ifidx, MOSRX_PKT_RX_QUEUE_SIDE, &sv) == 0) {
		d.has |= 8u;
		d.side_n = sv.n;
		d.side_same = sv.fhash == fh && sv.match == mt && sv.tcpinfo == ti && sv.n == v.n;
	}
	if (c->log && c->log_n < c->log_cap)
		c->log[c->log_n] = d;
	c->log_n++;
}

io_module_func hub_side_func = {
	.send_pkts = stub_send_pkts,
	.get_rptr = stub_get_rptr,
	.recv_pkts = stub_recv_pkts,
	.dev_ioctl = stub_dev_ioctl,
};
