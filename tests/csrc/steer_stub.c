/*
 * steer_stub.c — a stand-in io_module_func for mosrx_rx_loop_queues' CPU test
 * (tests/test_steer.py): it exposes the batches the test set, one per
 * recv_pkts, and serves their records and their steer view (computed by numpy)
 * through dev_ioctl; a consumer logs what the loop delivers.
 */
#include <stddef.h>
#include <string.h>

#include "mosrx_io_module.h"

typedef struct stub_batch {
	const uint8_t *frames;
	const uint32_t *off;
	const uint16_t *len;
	const void *res;            /* mosrx_result, or mosrx_result8 when compact */
	const uint32_t *idx;
	const uint32_t *qstart;
	uint32_t n;
	uint32_t compact;
} stub_batch;

typedef struct stub_delivery {
	uint64_t arg;
	int32_t ifidx, index;
	uint32_t len;
	uint8_t queue, first_byte;
	uint16_t batch;
} stub_delivery;

static const stub_batch *g_b;
static uint32_t g_nb, g_next, g_num_queues, g_steer = 1;
static int g_cur = -1;
static stub_delivery *g_log;
static uint32_t g_log_cap, g_log_n, g_sends;

void steer_stub_set(const stub_batch *b, uint32_t nb, uint32_t num_queues, int steer, stub_delivery *log,
                    uint32_t log_cap)
{
	g_b = b;
	g_nb = nb;
	g_next = 0;
	g_cur = -1;
	g_num_queues = num_queues;
	g_steer = (uint32_t)steer;
	g_log = log;
	g_log_cap = log_cap;
	g_log_n = 0;
	g_sends = 0;
}

uint32_t steer_stub_delivered(void) { return g_log_n; }
uint32_t steer_stub_sends(void) { return g_sends; }

static int32_t stub_recv_pkts(struct mtcp_thread_context *ctx, int ifidx)
{
	(void)ctx;
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
	const stub_batch *b;
	(void)ctx;
	if (ifidx != 0 || g_cur < 0 || index < 0 || (uint32_t)index >= g_b[g_cur].n)
		return NULL;
	b = &g_b[g_cur];
	*len = b->len[index];
	return (uint8_t *)(uintptr_t)(b->frames + b->off[index]);
}

static int32_t stub_send_pkts(struct mtcp_thread_context *ctx, int nif)
{
	(void)ctx;
	(void)nif;
	g_sends++;
	return 0;
}

static int32_t stub_dev_ioctl(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp)
{
	const stub_batch *b;
	(void)ctx;
	if (nif != 0 || g_cur < 0 || !argp)
		return -1;
	b = &g_b[g_cur];
	switch (cmd) {
	case MOSRX_PKT_RX_RESULTS:
		if (b->compact)
			return -1;
		*(const mosrx_result **)argp = b->res;
		return 0;
	case MOSRX_PKT_RX_RESULTS8:
		if (!b->compact)
			return -1;
		*(const mosrx_result8 **)argp = b->res;
		return 0;
	case MOSRX_PKT_RX_STEER: {
		mosrx_steer_view *v = argp;
		if (!g_steer)
			return -1;
		v->idx = b->idx;
		v->qstart = b->qstart;
		v->n = b->n;
		v->num_queues = g_num_queues;
		return 0;
	}
	default:
		return -1;
	}
}

void steer_stub_consume(void *arg, int ifidx, int index, const uint8_t *pkt, uint16_t len, const mosrx_result *res)
{
	if (g_log && g_log_n < g_log_cap) {
		stub_delivery *d = &g_log[g_log_n];
		d->arg = (uint64_t)(uintptr_t)arg;
		d->ifidx = ifidx;
		d->index = index;
		d->len = len;
		d->queue = res->queue;
		d->first_byte = len ? pkt[0] : 0;
		d->batch = (uint16_t)g_cur;
	}
	g_log_n++;
}

io_module_func steer_stub_func = {
	.send_pkts = stub_send_pkts,
	.get_rptr = stub_get_rptr,
	.recv_pkts = stub_recv_pkts,
	.dev_ioctl = stub_dev_ioctl,
};
