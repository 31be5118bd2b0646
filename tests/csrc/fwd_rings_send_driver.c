/*
 * fwd_rings_send_driver.c — mosrx_fwd_rings_send (csrc/fwd_tx.c) over a stub
 * io_module_func that records every get_wptr / send_pkts call and can refuse a
 * TX buffer for chosen frames.  A program of its own (plain, or under
 * -fsanitize=address,undefined): the entry arrays are heap blocks that end at
 * the last live entry, and dropped frames' entries are poisoned, so a read
 * outside start .. start + count of a ring is caught either way.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mosrx_io_module.h"

#define MAX_EV 64
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct ev { int send, nif, len; uint8_t *buf; };
struct mtcp_thread_context { struct ev ev[MAX_EV]; int nev, ngw; uint64_t refuse; /* bit k: the k-th get_wptr returns NULL */ };

static uint8_t *stub_get_wptr(struct mtcp_thread_context *c, int nif, uint16_t len)
{
	const int k = c->ngw++;
	struct ev *e = &c->ev[c->nev++];
	CHECK(c->nev <= MAX_EV);
	e->send = 0;
	e->nif = nif;
	e->len = len;
	e->buf = (c->refuse >> k) & 1 ? NULL : malloc(len ? len : 1);
	return e->buf;
}

static int32_t stub_send_pkts(struct mtcp_thread_context *c, int nif)
{
	struct ev *e = &c->ev[c->nev++];
	CHECK(c->nev <= MAX_EV);
	e->send = 1;
	e->nif = nif;
	e->len = 0;
	e->buf = NULL;
	return 0;
}

static void ctx_reset(struct mtcp_thread_context *c, uint64_t refuse)
{
	int i;
	for (i = 0; i < c->nev; i++)
		free(c->ev[i].buf);
	memset(c, 0, sizeof(*c));
	c->refuse = refuse;
}

/* rings: 0 three frames; 1 empty; 2 two written + two dropped; 3 one written + one dropped (the arrays end before it) */
#define NRINGS 4
#define RING_CAP 512u
static const mosrx_fwd_ring RINGS[NRINGS] = {{0, 3, 0, 14}, {3, 0, 0, 0}, {3, 2, 2, 9}, {7, 1, 1, 2}};
static const struct { uint32_t off; uint16_t len; } LIVE[] = {
	{0 * RING_CAP + 2, 60}, {0 * RING_CAP + 66, 14}, {0 * RING_CAP + 82, 129},
	{2 * RING_CAP + 2, 100}, {2 * RING_CAP + 114, 17},
	{3 * RING_CAP + 2, 30}};
static const int LIVE_ENTRY[] = {0, 1, 2, 3, 4, 7};
#define NLIVE 6
#define NENT 8   /* entries 5, 6 are ring 2's dropped frames; entry 8 (ring 3's) is past the arrays */

int main(void)
{
	io_module_func iom;
	struct mtcp_thread_context *ctx = calloc(1, sizeof(*ctx));
	uint8_t *tx = malloc(NRINGS * RING_CAP);
	uint32_t *toff = malloc(NENT * sizeof(*toff));
	uint16_t *tlen = malloc(NENT * sizeof(*tlen));
	mosrx_fwd_ring *rings = malloc(sizeof(RINGS));
	mosrx_fwd_send_stats st;
	int i, k, rc;
	CHECK(ctx && tx && toff && tlen && rings);
	memset(&iom, 0, sizeof(iom));
	iom.get_wptr = stub_get_wptr;
	iom.send_pkts = stub_send_pkts;
	for (i = 0; i < (int)(NRINGS * RING_CAP); i++)
		tx[i] = (uint8_t)(i * 131 + (i >> 8));
	for (i = 0; i < NENT; i++) {
		toff[i] = 0xFFFFFFF0u;                  /* poison: a read of it copies from far outside tx */
		tlen[i] = 0xFFFF;
	}
	for (i = 0; i < NLIVE; i++) {
		toff[LIVE_ENTRY[i]] = LIVE[i].off;
		tlen[LIVE_ENTRY[i]] = LIVE[i].len;
	}
	memcpy(rings, RINGS, sizeof(RINGS));

	/* every frame gets a buffer: calls in ring order, one send_pkts after each non-empty ring, none for ring 1 */
	memset(&st, 0, sizeof(st));
	rc = mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, NRINGS, &st);
	CHECK(rc == NLIVE && st.sent == NLIVE && st.no_buffer == 0 && st.send_calls == 3);
	{
		static const int want_nif[] = {0, 0, 0, 0, 2, 2, 2, 3, 3};
		static const int want_send[] = {0, 0, 0, 1, 0, 0, 1, 0, 1};
		CHECK(ctx->nev == 9);
		for (i = k = 0; i < ctx->nev; i++) {
			CHECK(ctx->ev[i].nif == want_nif[i] && ctx->ev[i].send == want_send[i]);
			if (ctx->ev[i].send)
				continue;
			CHECK(ctx->ev[i].len == LIVE[k].len && ctx->ev[i].buf);
			CHECK(!memcmp(ctx->ev[i].buf, tx + LIVE[k].off, LIVE[k].len));
			k++;
		}
		CHECK(k == NLIVE);
	}

	/* no buffer for the 2nd frame of ring 0 and both of ring 2: counted, the walk goes on, ring 2 is still flushed */
	ctx_reset(ctx, (1u << 1) | (1u << 3) | (1u << 4));
	rc = mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, NRINGS, &st);
	CHECK(rc == 3 && st.sent == NLIVE + 3 && st.no_buffer == 3 && st.send_calls == 6);
	CHECK(ctx->nev == 9 && ctx->ngw == NLIVE);
	for (i = k = 0; i < ctx->nev; i++) {
		if (ctx->ev[i].send)
			continue;
		CHECK(ctx->ev[i].len == LIVE[k].len);
		CHECK((ctx->ev[i].buf == NULL) == (k == 1 || k == 3 || k == 4));
		if (ctx->ev[i].buf)
			CHECK(!memcmp(ctx->ev[i].buf, tx + LIVE[k].off, LIVE[k].len));
		k++;
	}
	CHECK(ctx->ev[6].send && ctx->ev[6].nif == 2);

	/* fewer rings: only they are walked; st may be NULL */
	ctx_reset(ctx, 0);
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, 2, NULL) == 3 && ctx->nev == 4);
	/* all rings empty: no call at all */
	ctx_reset(ctx, 0);
	for (i = 0; i < NRINGS; i++)
		rings[i].count = 0;
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, NRINGS, &st) == 0 && ctx->nev == 0 && st.send_calls == 6);
	memcpy(rings, RINGS, sizeof(RINGS));

	/* -EINVAL: nothing is called */
	CHECK(mosrx_fwd_rings_send(NULL, ctx, tx, toff, tlen, rings, NRINGS, &st) == -EINVAL);
	CHECK(mosrx_fwd_rings_send(&iom, NULL, tx, toff, tlen, rings, NRINGS, &st) == -EINVAL);
	CHECK(mosrx_fwd_rings_send(&iom, ctx, NULL, toff, tlen, rings, NRINGS, &st) == -EINVAL);
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, NULL, tlen, rings, NRINGS, &st) == -EINVAL);
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, NULL, rings, NRINGS, &st) == -EINVAL);
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, NULL, NRINGS, &st) == -EINVAL);
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, 0, &st) == -EINVAL);
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, MOSRX_FWD_MAX_NETDEVS + 1, &st) == -EINVAL);
	iom.get_wptr = NULL;
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, NRINGS, &st) == -EINVAL);
	iom.get_wptr = stub_get_wptr;
	iom.send_pkts = NULL;
	CHECK(mosrx_fwd_rings_send(&iom, ctx, tx, toff, tlen, rings, NRINGS, &st) == -EINVAL);
	CHECK(ctx->nev == 0 && st.sent == NLIVE + 3 && st.no_buffer == 3 && st.send_calls == 6);

	ctx_reset(ctx, 0);
	free(ctx);
	free(tx);
	free(toff);
	free(tlen);
	free(rings);
	printf("fwd_rings_send_driver ok\n");
	return 0;
}
