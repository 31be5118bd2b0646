/*
 * hub_side_driver.c — a stand-alone run of the hub (csrc/hub.c) over the side
 * stub backend (hub_side_stub.c), for host sanitizer builds: cores 1.. on
 * pthreads, the owner on the main thread, each through mosrx_rx_loop.  Every
 * frame's side values are functions of its batch and original index, so each
 * delivery is checked on its own.  Exit 0 and "hub_side_driver ok" when every
 * core found, through its endpoint, exactly the side values of its frames (and
 * -1 for the arrays a batch lacks), and only the main thread called the backend.
 */
#include <pthread.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "mosrx_io_module.h"

/* hub_side_stub.c */
typedef struct hub_side_batch {
	const uint8_t *frames, *qrec;
	const uint32_t *qoff;
	const uint16_t *qlen;
	const uint32_t *idx, *qstart, *qfhash, *qmatch;
	const mosrx_tcpinfo *qtcpinfo;
	uint32_t n, rec_bytes;
} hub_side_batch;
typedef struct hub_side_call {
	uint64_t tid;
	uint32_t what;
	int32_t cmd;
} hub_side_call;
typedef struct hub_side_delivery {
	uint32_t batch, orig;
	int32_t index;
	uint32_t has, fhash, match;
	mosrx_tcpinfo ti;
	uint32_t side_n, side_same;
} hub_side_delivery;
typedef struct hub_side_core {
	struct mtcp_thread_context *ep;
	int32_t (*dev_ioctl)(struct mtcp_thread_context *ctx, int nif, int cmd, void *argp);
	hub_side_delivery *log;
	uint32_t log_cap, log_n, bad;
} hub_side_core;
void hub_side_set(const hub_side_batch *b, uint32_t nb, int side, hub_side_call *calls, uint32_t calls_cap);
uint32_t hub_side_calls(void);
uint64_t hub_side_self(void);
void hub_side_consume(void *arg, int ifidx, int index, const uint8_t *pkt, uint16_t len, const mosrx_result *res);
extern io_module_func hub_side_func;

#define NB 6
#define NCORES 3
#define NQ 5            /* queues 3 and 4 have no core */
#define FRAME 64
#define MAX_ROUNDS 2000000
#define NCALLS 8192

static mosrx_hub *g_hub;
static hub_side_core g_core[NCORES];
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

/* frame i of batch k */
static uint32_t fh_of(uint32_t k, uint32_t i) { return (i + 1u) * 2654435761u + k; }
static uint32_t mt_of(uint32_t k, uint32_t i) { return (i * 40503u) ^ (k << 28) ^ 0xA5A5u; }
static mosrx_tcpinfo ti_of(uint32_t k, uint32_t i)
{
	mosrx_tcpinfo t = {i, ~i, (uint16_t)(i * 7u), (uint16_t)(k + 40u)};
	return t;
}
/* the arrays batch k has: all, no masks, no pkt_info, none */
static int has_fh(uint32_t k) { return k % 4 != 3; }
static int has_mt(uint32_t k) { return k % 4 == 0 || k % 4 == 2; }
static int has_ti(uint32_t k) { return k % 4 == 0 || k % 4 == 1; }

static void *core_main(void *a)
{
	const uint32_t c = (uint32_t)(uintptr_t)a;
	mosrx_rx_stats st;
	uint32_t r;
	for (r = 0; r < MAX_ROUNDS; r++) {
		if (mosrx_rx_loop(&mosrx_hub_module_func, g_core[c].ep, 1, 0, hub_side_consume, &g_core[c], &st)) {
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

static int run(int side)
{
	static const uint32_t ns[NB] = {6161, 65, 2049, 1, 700, 4096};
	hub_side_batch b[NB];
	static hub_side_call calls[NCALLS];
	uint64_t want[NCORES] = {0}, total = 0, owned = 0;
	pthread_t th[NCORES];
	mosrx_hub_stats hs;
	mosrx_rx_stats st;
	uint32_t seed = 4242, k, i, c, r, ncalls, nside = 0;
	int rc, bad = 0;
	atomic_store(&g_done, 0);
	for (k = 0; k < NB; k++) {
		const uint32_t n = ns[k];
		uint8_t *frames = calloc((size_t)n, FRAME), *key = malloc(n);
		mosrx_result *qrec = calloc(n, sizeof(*qrec));
		uint32_t *qoff = malloc((size_t)n * 4), *idx = malloc((size_t)n * 4), *qstart = calloc(MOSRX_STEER_QSLOTS, 4);
		uint32_t *qfh = has_fh(k) ? malloc((size_t)n * 4) : NULL, *qmt = has_mt(k) ? malloc((size_t)n * 4) : NULL;
		mosrx_tcpinfo *qti = has_ti(k) ? malloc((size_t)n * sizeof(*qti)) : NULL;
		uint16_t *qlen = malloc((size_t)n * 2);
		uint32_t pos[256];
		if (!frames || !key || !qrec || !qoff || !idx || !qstart || !qlen || (has_fh(k) && !qfh) ||
		    (has_mt(k) && !qmt) || (has_ti(k) && !qti))
			return 2;
		for (i = 0; i < n; i++) {
			key[i] = (uint8_t)(rnd(&seed) % NQ);
			qstart[key[i] + 1]++;
		}
		for (i = 0; i < 256; i++)
			qstart[i + 1] += qstart[i];
		for (i = 0; i < 256; i++)
			pos[i] = qstart[i];
		for (i = 0; i < n; i++) {   /* the stable partition and its gather, side arrays included */
			const uint32_t p = pos[key[i]]++;
			idx[p] = i;
			qoff[p] = i * FRAME;
			qlen[p] = FRAME;
			qrec[p].queue = key[i];
			qrec[p].verdict = 1;
			if (qfh)
				qfh[p] = fh_of(k, i);
			if (qmt)
				qmt[p] = mt_of(k, i);
			if (qti)
				qti[p] = ti_of(k, i);
		}
		b[k] = (hub_side_batch){frames, (const uint8_t *)qrec, qoff, qlen, idx, qstart, qfh, qmt, qti, n,
		                        sizeof(mosrx_result)};
		for (c = 0; c < NCORES; c++)
			want[c] += qstart[c + 1] - qstart[c];
		owned += qstart[NCORES];
		total += n;
		free(key);
	}
	hub_side_set(b, NB, side, calls, NCALLS);
	if ((rc = mosrx_hub_open(&hub_side_func, NULL, 1, NCORES, &g_hub))) {
		printf("mosrx_hub_open %d\n", rc);
		return 1;
	}
	for (c = 0; c < NCORES; c++) {
		memset(&g_core[c], 0, sizeof(g_core[c]));
		g_fail[c] = 0;
		g_core[c].ep = mosrx_hub_endpoint(g_hub, c);
		g_core[c].dev_ioctl = mosrx_hub_module_func.dev_ioctl;
		g_core[c].log_cap = (uint32_t)want[c];
		if (!(g_core[c].log = calloc(want[c] + 1, sizeof(hub_side_delivery))))
			return 2;
	}
	for (c = 1; c < NCORES; c++)
		if (pthread_create(&th[c], NULL, core_main, (void *)(uintptr_t)c))
			return 2;
	for (r = 0; r < MAX_ROUNDS; r++) {
		mosrx_hub_stats h0, h1;
		mosrx_hub_stats_get(g_hub, &h0);
		if (mosrx_rx_loop(&mosrx_hub_module_func, g_core[0].ep, 1, 0, hub_side_consume, &g_core[0], &st))
			bad |= 2;
		mosrx_hub_stats_get(g_hub, &h1);
		/* an idle round that was the backend's own: every share of the last batch went back */
		if (h1.frames == total && h1.batches == h0.batches && h1.owner_waits == h0.owner_waits)
			break;
		if (!st.rx_packets)
			usleep(20);
	}
	if (r == MAX_ROUNDS)
		bad |= 4;
	atomic_store(&g_done, 1);
	for (c = 1; c < NCORES; c++)
		pthread_join(th[c], NULL);
	for (c = 0; c < NCORES; c++) {
		if (g_fail[c] || g_core[c].bad || g_core[c].log_n != want[c])
			bad |= 8;
		for (i = 0; i < g_core[c].log_n && i < g_core[c].log_cap; i++) {
			const hub_side_delivery *d = &g_core[c].log[i];
			const uint32_t kk = d->batch;
			const mosrx_tcpinfo t = ti_of(kk, d->orig);
			const uint32_t has = !side ? 0u : 8u | (has_fh(kk) ? 1u : 0u) | (has_mt(kk) ? 2u : 0u) | (has_ti(kk) ? 4u : 0u);
			if (kk >= NB || d->has != has || (side && !d->side_same)) {
				bad |= 16;
				continue;
			}
			if (((has & 1u) && d->fhash != fh_of(kk, d->orig)) || ((has & 2u) && d->match != mt_of(kk, d->orig)) ||
			    ((has & 4u) && memcmp(&d->ti, &t, sizeof(t))))
				bad |= 32;
		}
	}
	mosrx_hub_stats_get(g_hub, &hs);
	if (hs.batches != NB || hs.frames != total || hs.delivered != owned || hs.unowned != total - owned)
		bad |= 64;
	ncalls = hub_side_calls();
	if (ncalls > NCALLS)
		bad |= 128;
	for (i = 0; i < ncalls && i < NCALLS; i++) {
		if (calls[i].tid != hub_side_self() || calls[i].what == 4)
			bad |= 256;
		if (calls[i].what == 2 && calls[i].cmd == MOSRX_PKT_RX_QUEUE_SIDE)
			nside++;
	}
	/* the probe, then one view per core and batch -- or the probe alone over a backend without them */
	if (nside != (side ? 1u + NB * NCORES : 1u))
		bad |= 512;
	if (mosrx_hub_close(g_hub))
		bad |= 1024;
	for (c = 0; c < NCORES; c++)
		free(g_core[c].log);
	for (k = 0; k < NB; k++) {
		free((void *)(uintptr_t)b[k].frames);
		free((void *)(uintptr_t)b[k].qrec);
		free((void *)(uintptr_t)b[k].qoff);
		free((void *)(uintptr_t)b[k].qlen);
		free((void *)(uintptr_t)b[k].idx);
		free((void *)(uintptr_t)b[k].qstart);
		free((void *)(uintptr_t)b[k].qfhash);
		free((void *)(uintptr_t)b[k].qmatch);
		free((void *)(uintptr_t)b[k].qtcpinfo);
	}
	if (bad)
		printf("hub_side_driver FAILED (side %d): %#x\n", side, bad);
	return bad ? 1 : 0;
}

int main(void)
{
	if (run(1) || run(0))
		return 1;
	printf("hub_side_driver ok\n");
	return 0;
}
