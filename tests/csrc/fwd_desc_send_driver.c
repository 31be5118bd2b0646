/*
 * fwd_desc_send_driver.c — mosrx_fwd_desc_send (csrc/fwd_tx.c) over a stub
 * io_module_func that records every get_wptr / send_pkts call and can refuse a
 * TX buffer for chosen frames, compared call by call and byte by byte with
 * mosrx_fwd_rings_send over the byte rings of the same entries.  A program of
 * its own (plain, or under -fsanitize=address,undefined): the entry arrays are
 * heap blocks that end at the last live entry, and the entries between the
 * rings are poisoned (a source index far outside off[], the longest length), so
 * a read outside start .. start + count of a ring is caught either way.
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

/* the received batch: NSRC frames at every offset mod 4, the last ending exactly at the buffer's end */
#define NSRC 9
static const uint32_t SRC_OFF[NSRC] = {0, 61, 130, 207, 300, 330, 470, 601, 750};
static const uint16_t SRC_LEN[NSRC] = {60, 64, 70, 90, 14, 129, 100, 140, 34};
#define FRAMES_BYTES (750 + 34)

/* 16 rings: 0 three frames; 1 empty; 2 two; 5 one (two poisoned entries before it); 15 two; the rest empty */
#define NRINGS 16
#define RING_CAP 512u
#define NENT 10
static const struct { uint32_t q, e, src; uint16_t len; } LIVE[] = {
	{0, 0, 3, 90}, {0, 1, 4, 14}, {0, 2, 0, 46},
	{2, 3, 7, 140}, {2, 4, 1, 64},
	{5, 7, 8, 34},
	{15, 8, 5, 129}, {15, 9, 2, 70}};
#define NLIVE 8

static void same_events(const struct mtcp_thread_context *a, const struct mtcp_thread_context *b)
{
	int i;
	CHECK(a->nev == b->nev && a->ngw == b->ngw);
	for (i = 0; i < a->nev; i++) {
		const struct ev *x = &a->ev[i], *y = &b->ev[i];
		CHECK(x->send == y->send && x->nif == y->nif && x->len == y->len && !x->buf == !y->buf);
		if (x->buf)
			CHECK(!memcmp(x->buf, y->buf, (size_t)x->len));
	}
}

int main(void)
{
	io_module_func iom;
	struct mtcp_thread_context *ca = calloc(1, sizeof(*ca)), *cb = calloc(1, sizeof(*cb));
	uint8_t *frames = malloc(FRAMES_BYTES);
	uint32_t *off = malloc(NSRC * sizeof(*off));
	uint8_t *tx = malloc(NRINGS * RING_CAP);
	uint32_t *toff = malloc(NENT * sizeof(*toff)), *tsrc = malloc(NENT * sizeof(*tsrc));
	uint16_t *tlen = malloc(NENT * sizeof(*tlen));
	uint32_t *tmac = malloc(NENT * 12);
	mosrx_fwd_ring *rings = calloc(NRINGS, sizeof(*rings)), *saved = calloc(NRINGS, sizeof(*rings));
	mosrx_fwd_send_stats sa, sb;
	uint32_t fill[NRINGS] = {0};
	int i, k, ra, rb;
	CHECK(ca && cb && frames && off && tx && toff && tsrc && tlen && tmac && rings && saved);
	memset(&iom, 0, sizeof(iom));
	iom.get_wptr = stub_get_wptr;
	iom.send_pkts = stub_send_pkts;
	for (i = 0; i < FRAMES_BYTES; i++)
		frames[i] = (uint8_t)(i * 131 + (i >> 8));
	memcpy(off, SRC_OFF, sizeof(SRC_OFF));
	CHECK(SRC_OFF[NSRC - 1] + SRC_LEN[NSRC - 1] == FRAMES_BYTES);
	memset(tx, 0xEE, NRINGS * RING_CAP);
	for (i = 0; i < NENT; i++) {
		toff[i] = 0xFFFFFFF0u;                  /* poison: a read of it copies from far outside */
		tsrc[i] = 0xFFFFFFF0u;
		tlen[i] = 0xFFFF;
		memset(tmac + 3 * i, 0xEE, 12);
	}
	/* both forms of the same entries: the byte ring holds tx_mac followed by the frame's bytes 12 .. len */
	for (i = 0; i < NLIVE; i++) {
		const uint32_t q = LIVE[i].q, e = LIVE[i].e, s = LIVE[i].src, len = LIVE[i].len;
		uint8_t mac[12];
		uint8_t *w = tx + q * RING_CAP + 16 * fill[q] + 2;
		CHECK(len >= 14 && len <= SRC_LEN[s] && 16 * fill[q] + 2 + len <= RING_CAP);
		for (k = 0; k < 12; k++)
			mac[k] = (uint8_t)(0xA0 + 16 * i + k);
		memcpy(tmac + 3 * e, mac, 12);
		tsrc[e] = s;
		tlen[e] = (uint16_t)len;
		toff[e] = (uint32_t)(w - tx);
		memcpy(w, mac, 12);
		memcpy(w + 12, frames + SRC_OFF[s] + 12, len - 12);
		if (!rings[q].count)
			rings[q].start = e;
		rings[q].count++;
		fill[q] += (2 + len + 15) / 16;
		rings[q].units = fill[q];
	}
	memcpy(saved, rings, NRINGS * sizeof(*rings));

	/* every frame gets a buffer: the same calls and bytes as the byte rings', one send_pkts per non-empty ring */
	memset(&sa, 0, sizeof(sa));
	memset(&sb, 0, sizeof(sb));
	ra = mosrx_fwd_rings_send(&iom, ca, tx, toff, tlen, rings, NRINGS, &sa);
	rb = mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, NRINGS, &sb);
	CHECK(ra == NLIVE && rb == NLIVE && !memcmp(&sa, &sb, sizeof(sa)) && sb.sent == NLIVE && sb.send_calls == 4);
	CHECK(cb->nev == NLIVE + 4);
	same_events(ca, cb);
	for (i = k = 0; i < cb->nev; i++) {
		if (cb->ev[i].send)
			continue;
		CHECK(cb->ev[i].nif == (int)LIVE[k].q && cb->ev[i].len == LIVE[k].len);
		CHECK(!memcmp(cb->ev[i].buf, tmac + 3 * LIVE[k].e, 12));
		CHECK(!memcmp(cb->ev[i].buf + 12, frames + SRC_OFF[LIVE[k].src] + 12, (size_t)LIVE[k].len - 12));
		k++;
	}
	CHECK(k == NLIVE && cb->ev[cb->nev - 1].send && cb->ev[cb->nev - 1].nif == 15);

	/* no buffer in the middle of ring 0, for ring 2's first and ring 15's last: counted, the walk goes on */
	ctx_reset(ca, (1u << 1) | (1u << 3) | (1u << 7));
	ctx_reset(cb, (1u << 1) | (1u << 3) | (1u << 7));
	ra = mosrx_fwd_rings_send(&iom, ca, tx, toff, tlen, rings, NRINGS, &sa);
	rb = mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, NRINGS, &sb);
	CHECK(ra == NLIVE - 3 && rb == ra && !memcmp(&sa, &sb, sizeof(sa)));
	CHECK(sb.sent == 2 * NLIVE - 3 && sb.no_buffer == 3 && sb.send_calls == 8 && cb->ngw == NLIVE);
	same_events(ca, cb);
	CHECK(!cb->ev[1].buf && cb->ev[2].buf && cb->ev[3].send);

	/* fewer rings: only they are walked; st may be NULL */
	ctx_reset(cb, 0);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, 3, NULL) == 5 && cb->nev == 7);
	/* all rings empty: no call at all */
	ctx_reset(cb, 0);
	for (i = 0; i < NRINGS; i++)
		rings[i].count = 0;
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, NRINGS, &sb) == 0 && cb->nev == 0 &&
	      sb.send_calls == 8);
	memcpy(rings, saved, NRINGS * sizeof(*rings));

	/* -EINVAL: nothing is called */
	CHECK(mosrx_fwd_desc_send(NULL, cb, frames, off, tsrc, tlen, tmac, rings, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, NULL, frames, off, tsrc, tlen, tmac, rings, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, NULL, off, tsrc, tlen, tmac, rings, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, NULL, tsrc, tlen, tmac, rings, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, NULL, tlen, tmac, rings, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, NULL, tmac, rings, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, NULL, rings, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, NULL, NRINGS, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, 0, &sb) == -EINVAL);
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, MOSRX_FWD_MAX_NETDEVS + 1, &sb) == -EINVAL);
	iom.get_wptr = NULL;
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, NRINGS, &sb) == -EINVAL);
	iom.get_wptr = stub_get_wptr;
	iom.send_pkts = NULL;
	CHECK(mosrx_fwd_desc_send(&iom, cb, frames, off, tsrc, tlen, tmac, rings, NRINGS, &sb) == -EINVAL);
	CHECK(cb->nev == 0 && sb.sent == 2 * NLIVE - 3 && sb.no_buffer == 3 && sb.send_calls == 8);

	ctx_reset(ca, 0);
	ctx_reset(cb, 0);
	free(ca);
	free(cb);
	free(frames);
	free(off);
	free(tx);
	free(toff);
	free(tsrc);
	free(tlen);
	free(tmac);
	free(rings);
	free(saved);
	printf("fwd_desc_send_driver ok\n");
	return 0;
}
