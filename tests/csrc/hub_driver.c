/*
 * hub_driver.c — a stand-alone run of the hub (csrc/hub.c) over the stub
 * backend (hub_stub.c), for host sanitizer builds: cores 1.. on pthreads, the
 * owner on the main thread, each through mosrx_rx_loop.  Exit 0 and
 * "hub_driver ok" when every core consumed exactly its partition, only the
 * main thread called the backend, and no recv_pkts arrived while a share was
 * outstanding.
 */
#include <pthread.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "mosrx_io_module.h"

/* hub_stub.c */
typedef struct hub_stub_batch {
	const uint8_t *frames, *qrec;
	const uint32_t *qoff;
	const uint16_t *qlen;
	const uint32_t *idx, *qstart;
	uint32_t n, rec_bytes;
} hub_stub_batch;
typedef struct hub_stub_call {
	uint64_t tid, consumed;
	uint32_t what;
	int32_t cur;
} hub_stub_call;
typedef struct hub_stub_core {
	struct mtcp_thread_context *ep;
	int32_t (*dev_ioctl)(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp);
	void *log;
	uint32_t log_cap, log_n, sleep_us, sleep_every, bad;
} hub_stub_core;
void hub_stub_set(const hub_stub_batch *b, uint32_t nb, int gather, hub_stub_call *calls, uint32_t calls_cap);
uint32_t hub_stub_calls(void);
uint32_t hub_stub_exhausted(void);
uint64_t hub_stub_self(void);
void hub_stub_consume(void *arg, int ifidx, int index, const uint8_t *pkt, uint16_t len, const mosrx_result *res);
extern io_module_func hub_stub_func;

#define NB 6
#define NCORES 3
#define NQ 5            /* queues 3 and 4 have no core */
#define FRAME 64
#define MAX_ROUNDS 2000000

static mosrx_hub *g_hub;
static hub_stub_core g_core[NCORES];
static atomic_int g_done;
static int g_fail[NCORES];

/* rx_loop.c's latency probe asks the paced source for its clock; no source is linked here */
int mosrx_source_paced_info(const mosrx_source *s, uint64_t *t0_ns, double *ns_per_frame, uint64_t *released)
{
	(void)s;
	(void)t0_ns;
	(void)ns_per_frame;
	(void)released;
	return -1;
}

static uint32_t rnd(uint32_t *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

static void *core_main(void *a)
{
	const uint32_t c = (uint32_t)(uintptr_t)a;
	mosrx_rx_stats st;
	uint32_t r;
	for (r = 0; r < MAX_ROUNDS; r++) {
		if (mosrx_rx_loop(&mosrx_hub_module_func, g_core[c].ep, 1, 0, hub_stub_consume, &g_core[c], &st)) {
			g_fail[c] = 1;
			return NULL;
		}
		if (atomic_load(&g_done))
			return NULL;
		if (!st.rx_packets)
			usleep(50);
	}
	g_fail[c] = 2;
	return NULL;
}

int main(void)
{
	static const uint32_t ns[NB] = {6161, 65, 2049, 1, 700, 4096};
	hub_stub_batch b[NB];
	static hub_stub_call calls[4096];
	uint64_t want[NCORES] = {0}, owned_cum[NB + 1] = {0}, total = 0;
	pthread_t th[NCORES];
	mosrx_hub_stats hs;
	mosrx_rx_stats st;
	uint32_t seed = 12345, k, i, c, r, nrecv = 0, ncalls;
	int rc, bad = 0;
	for (k = 0; k < NB; k++) {
		const uint32_t n = ns[k];
		uint8_t *frames = malloc((size_t)n * FRAME), *key = malloc(n);
		mosrx_result *qrec = calloc(n, sizeof(*qrec));
		uint32_t *qoff = malloc((size_t)n * 4), *idx = malloc((size_t)n * 4), *qstart = calloc(MOSRX_STEER_QSLOTS, 4);
		uint16_t *qlen = malloc((size_t)n * 2);
		uint32_t pos[256];
		if (!frames || !key || !qrec || !qoff || !idx || !qstart || !qlen)
			return 2;
		for (i = 0; i < n * FRAME; i++)
			frames[i] = (uint8_t)rnd(&seed);
		for (i = 0; i < n; i++) {
			key[i] = (uint8_t)(rnd(&seed) % NQ);
			qstart[key[i] + 1]++;
		}
		for (i = 0; i < 256; i++)
			qstart[i + 1] += qstart[i];
		for (i = 0; i < 256; i++)
			pos[i] = qstart[i];
		for (i = 0; i < n; i++) {   /* the stable partition and its gather */
			const uint32_t p = pos[key[i]]++;
			idx[p] = i;
			qoff[p] = i * FRAME;
			qlen[p] = FRAME;
			qrec[p].queue = key[i];
			qrec[p].verdict = 1;
			qrec[p].rss = i;
		}
		b[k] = (hub_stub_batch){frames, (const uint8_t *)qrec, qoff, qlen, idx, qstart, n, sizeof(mosrx_result)};
		for (c = 0; c < NCORES; c++)
			want[c] += qstart[c + 1] - qstart[c];
		owned_cum[k + 1] = owned_cum[k] + qstart[NCORES];
		total += n;
		free(key);
	}
	hub_stub_set(b, NB, 1, calls, 4096);
	if ((rc = mosrx_hub_open(&hub_stub_func, NULL, 1, NCORES, &g_hub))) {
		printf("mosrx_hub_open %d\n", rc);
		return 1;
	}
	for (c = 0; c < NCORES; c++) {
		memset(&g_core[c], 0, sizeof(g_core[c]));
		g_core[c].ep = mosrx_hub_endpoint(g_hub, c);
		g_core[c].dev_ioctl = mosrx_hub_module_func.dev_ioctl;
		if (c == NCORES - 1) {
			g_core[c].sleep_us = 100;
			g_core[c].sleep_every = 16;
		}
	}
	for (c = 1; c < NCORES; c++)
		if (pthread_create(&th[c], NULL, core_main, (void *)(uintptr_t)c))
			return 2;
	if (mosrx_rx_loop(&mosrx_hub_module_func, g_core[0].ep, 1, 1, hub_stub_consume, &g_core[0], &st) ||
	    mosrx_hub_close(g_hub) != -16)
		bad |= 1;
	for (r = 0; r < MAX_ROUNDS && !hub_stub_exhausted(); r++) {
		if (mosrx_rx_loop(&mosrx_hub_module_func, g_core[0].ep, 1, 0, hub_stub_consume, &g_core[0], &st))
			bad |= 2;
		if (!st.rx_packets)
			usleep(20);
	}
	atomic_store(&g_done, 1);
	for (c = 1; c < NCORES; c++)
		pthread_join(th[c], NULL);
	if (!hub_stub_exhausted())
		bad |= 4;
	for (c = 0; c < NCORES; c++)
		if (g_fail[c] || g_core[c].bad || g_core[c].log_n != want[c])
			bad |= 8;
	mosrx_hub_stats_get(g_hub, &hs);
	if (hs.batches != NB || hs.frames != total || hs.delivered != owned_cum[NB] ||
	    hs.unowned != total - owned_cum[NB] || hs.unowned == 0)
		bad |= 16;
	ncalls = hub_stub_calls();
	for (i = 0; i < ncalls && i < 4096; i++) {
		if (calls[i].tid != hub_stub_self() || calls[i].what == 4)
			bad |= 32;
		if (calls[i].what == 1) {
			if (nrecv > NB || calls[i].consumed != owned_cum[nrecv])
				bad |= 64;
			nrecv++;
		}
	}
	if (nrecv != NB + 1)
		bad |= 128;
	if (mosrx_hub_close(g_hub))
		bad |= 256;
	for (k = 0; k < NB; k++) {
		free((void *)(uintptr_t)b[k].frames);
		free((void *)(uintptr_t)b[k].qrec);
		free((void *)(uintptr_t)b[k].qoff);
		free((void *)(uintptr_t)b[k].qlen);
		free((void *)(uintptr_t)b[k].idx);
		free((void *)(uintptr_t)b[k].qstart);
	}
	if (bad) {
		printf("hub_driver FAILED: %#x\n", bad);
		return 1;
	}
	printf("hub_driver ok: %u batches, %llu frames, %llu unowned, %llu owner waits\n", NB,
	       (unsigned long long)total, (unsigned long long)hs.unowned, (unsigned long long)hs.owner_waits);
	return 0;
}
