/*
 * nat_table.c — the NAT lookup table's arithmetic (include/mosrx.h): its hash
 * and size, the build from a binding array, and bindings added and removed in
 * place with delete markers.  Plain C over host memory: no GPU, no HIP header,
 * so the stand-alone driver (tests/csrc/nat_update_driver.c) compiles this file
 * as it is.  nat_api.c keeps the context's side.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "mosrx_nat.h"

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

/* The two keys of a binding (include/mosrx.h): client side, server side. */
#define CLI_KEY(x) (x)->cli_ip, (x)->svr_ip, ((uint32_t)(x)->cli_port | (uint32_t)(x)->svr_port << 16)
#define SVR_KEY(x) (x)->svr_ip, (x)->nat_ip, ((uint32_t)(x)->svr_port | (uint32_t)(x)->nat_port << 16)

int mosrx__nat_build_ids(const mosrx_nat_binding *b, const uint32_t *ids, uint32_t n, mosrx_nat_slot *slots, uint32_t cap,
                         uint32_t *probe)
{
	uint32_t i, run = 0, mask;
	if (n > MOSRX_NAT_MAX_BINDINGS || (n && !b) || !slots || (cap && (cap < mosrx_nat_slots(n) || (cap & (cap - 1)))))
		return -EINVAL;
	mask = (cap ? cap : mosrx_nat_slots(n)) - 1;
	memset(slots, 0, ((size_t)mask + 1) * sizeof(*slots));
	for (i = 0; i < n; i++) {
		const mosrx_nat_binding *x = &b[i];
		const uint32_t id = ids ? ids[i] : i;
		if (!x->nat_ip || !x->nat_port)
			return -EINVAL;
		/* client side: the frame the client sent; server side: the server's answer to the NAT's address */
		if (nat_insert(slots, mask, CLI_KEY(x), MOSRX_NAT_SNAT, x->nat_ip, x->nat_port, id, &run) ||
		    nat_insert(slots, mask, SVR_KEY(x), MOSRX_NAT_DNAT, x->cli_ip, x->cli_port, id, &run))
			return -EINVAL;
	}
	if (probe)
		*probe = run;
	return 0;
}

int mosrx_nat_build(const mosrx_nat_binding *b, uint32_t n, mosrx_nat_slot *slots, uint32_t *probe)
{
	return mosrx__nat_build_ids(b, NULL, n, slots, 0, probe);
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

uint32_t mosrx__nat_live(const mosrx_nat_slot *slots, uint32_t nslots, mosrx_nat_binding *b, uint32_t *ids, uint32_t max)
{
	uint32_t i, n = 0;
	for (i = 0; i < nslots; i++) {
		const mosrx_nat_slot *s = &slots[i];
		if (s->kind != MOSRX_NAT_SNAT)
			continue;
		if (n < max) {
			memset(&b[n], 0, sizeof(b[n]));
			b[n].cli_ip = s->saddr;
			b[n].svr_ip = s->daddr;
			b[n].cli_port = (uint16_t)s->ports;
			b[n].svr_port = (uint16_t)(s->ports >> 16);
			b[n].nat_ip = s->addr;
			b[n].nat_port = s->port;
			ids[n] = s->bind;
		}
		n++;
	}
	return n;
}

/* ---- bindings added and removed in place ------------------------------------------- */

/* A table's changes as they are made: each write's slot and the image it
 * replaces go to the caller's touch array, which so serves as the undo list of a
 * refused call before it becomes the answer of an accepted one. */
struct nat_edit {
	mosrx_nat_slot *slots;
	uint32_t mask;
	mosrx_nat_tstate st;
	mosrx_nat_touch *log;
	uint32_t nlog;
};

static mosrx_nat_slot *nat_edit_slot(struct nat_edit *e, uint32_t at)
{
	mosrx_nat_touch *t = &e->log[e->nlog++];   /* (two writes an op at most: 2 n <= 4 n entries) */
	memset(t, 0, sizeof(*t));
	t->slot = at;
	t->image = e->slots[at];
	return &e->slots[at];
}

/* The walk of a lookup that steps over delete markers: the slot of the live key,
 * or -1 where a free slot (or the table's end of slots) shows it absent.  With
 * first_tomb / free_at the places an insert may take (their distances + 1 in
 * *need: what probe must cover), -1 where there is none. */
static int64_t nat_find(const struct nat_edit *e, uint32_t sa, uint32_t da, uint32_t pt, int64_t *first_tomb,
                        int64_t *free_at, uint32_t *tomb_need, uint32_t *free_need)
{
	const uint32_t h = mosrx_nat_hash_key(sa, da, pt);
	uint32_t d;
	if (first_tomb)
		*first_tomb = *free_at = -1;
	for (d = 0; d <= e->mask; d++) {
		const uint32_t at = (h + d) & e->mask;
		const mosrx_nat_slot *s = &e->slots[at];
		if (!s->kind) {
			if (first_tomb) {
				*free_at = at;
				*free_need = d + 1;
			}
			return -1;
		}
		if (s->kind == MOSRX_NAT_TOMB) {
			if (first_tomb && *first_tomb < 0) {
				*first_tomb = at;
				*tomb_need = d + 1;
			}
			continue;
		}
		if (s->saddr == sa && s->daddr == da && s->ports == pt)
			return at;
	}
	return -1;
}

static int nat_edit_add_key(struct nat_edit *e, uint32_t sa, uint32_t da, uint32_t pt, uint8_t kind, uint32_t addr,
                            uint16_t port, uint32_t bind)
{
	int64_t tomb, fre;
	uint32_t tomb_need = 0, free_need = 0, need;
	mosrx_nat_slot *s;
	if (nat_find(e, sa, da, pt, &tomb, &fre, &tomb_need, &free_need) >= 0)
		return -EEXIST;
	if (tomb >= 0) {
		s = nat_edit_slot(e, (uint32_t)tomb);
		need = tomb_need;
		e->st.tombs--;
	} else {
		/* (fre < 0: no free slot in the whole table, which a table at most half full always has) */
		if (fre < 0 || e->st.keys + e->st.tombs + 1 > (e->mask + 1) / 2)
			return -ENOSPC;
		s = nat_edit_slot(e, (uint32_t)fre);
		need = free_need;
	}
	memset(s, 0, sizeof(*s));
	s->saddr = sa;
	s->daddr = da;
	s->ports = pt;
	s->port = port;
	s->kind = kind;
	s->addr = addr;
	s->bind = bind;
	e->st.keys++;
	if (need > e->st.probe)
		e->st.probe = need;
	return 0;
}

static int nat_edit_op(struct nat_edit *e, const mosrx_nat_op *o)
{
	const mosrx_nat_binding *x = &o->b;
	int rc;
	if ((o->op != MOSRX_NAT_OP_ADD && o->op != MOSRX_NAT_OP_DEL) || !x->nat_ip || !x->nat_port)
		return -EINVAL;
	if (o->op == MOSRX_NAT_OP_ADD) {
		if (o->bind == MOSRX_NAT_NO_BIND)
			return -EINVAL;
		if (nat_find(e, CLI_KEY(x), NULL, NULL, NULL, NULL) >= 0 || nat_find(e, SVR_KEY(x), NULL, NULL, NULL, NULL) >= 0)
			return -EEXIST;
		/* (before -ENOSPC: a rebuild would not make room for it either) */
		if (e->st.keys / 2 + 1 > MOSRX_NAT_MAX_BINDINGS)
			return -EINVAL;
		if ((rc = nat_edit_add_key(e, CLI_KEY(x), MOSRX_NAT_SNAT, x->nat_ip, x->nat_port, o->bind)))
			return rc;
		/* (-EEXIST here: the binding's own two keys are one) */
		return nat_edit_add_key(e, SVR_KEY(x), MOSRX_NAT_DNAT, x->cli_ip, x->cli_port, o->bind);
	}
	{
		const int64_t ca = nat_find(e, CLI_KEY(x), NULL, NULL, NULL, NULL), sa = nat_find(e, SVR_KEY(x), NULL, NULL, NULL, NULL);
		const mosrx_nat_slot *cs, *ss;
		mosrx_nat_slot *s;
		if (ca < 0 || sa < 0 || ca == sa)
			return -ENOENT;
		cs = &e->slots[ca];
		ss = &e->slots[sa];
		if (cs->kind != MOSRX_NAT_SNAT || cs->addr != x->nat_ip || cs->port != x->nat_port || ss->kind != MOSRX_NAT_DNAT ||
		    ss->addr != x->cli_ip || ss->port != x->cli_port || cs->bind != ss->bind)
			return -ENOENT;
		s = nat_edit_slot(e, (uint32_t)ca);
		memset(s, 0, sizeof(*s));
		s->kind = MOSRX_NAT_TOMB;
		s = nat_edit_slot(e, (uint32_t)sa);
		memset(s, 0, sizeof(*s));
		s->kind = MOSRX_NAT_TOMB;
		e->st.keys -= 2;
		e->st.tombs += 2;
	}
	return 0;
}

static int touch_by_slot(const void *a, const void *b)
{
	const uint32_t x = ((const mosrx_nat_touch *)a)->slot, y = ((const mosrx_nat_touch *)b)->slot;
	return x < y ? -1 : x > y;
}

int mosrx_nat_apply(mosrx_nat_slot *slots, mosrx_nat_tstate *st, const mosrx_nat_op *ops, uint32_t n,
                    mosrx_nat_touch *touch, uint32_t *ntouch)
{
	struct nat_edit e;
	uint32_t i, m;
	int rc = 0;
	if (!slots || !st || !ntouch || (n && (!ops || !touch)) || n > 0x3FFFFFFFu || st->slots < MOSRX_NAT_MIN_SLOTS ||
	    (st->slots & (st->slots - 1)) || st->keys > st->slots / 2 || st->tombs > st->slots / 2 - st->keys ||
	    st->probe > st->slots)
		return -EINVAL;
	e.slots = slots;
	e.mask = st->slots - 1;
	e.st = *st;
	e.log = touch;
	e.nlog = 0;
	for (i = 0; i < n && !rc; i++)
		rc = nat_edit_op(&e, &ops[i]);
	if (rc) {
		/* undo, last write first */
		while (e.nlog) {
			const mosrx_nat_touch *t = &touch[--e.nlog];
			slots[t->slot] = t->image;
		}
		return rc;
	}
	/* one entry a slot, ascending, with the slot's final image */
	qsort(touch, e.nlog, sizeof(*touch), touch_by_slot);
	for (i = 0, m = 0; i < e.nlog; i++) {
		if (m && touch[m - 1].slot == touch[i].slot)
			continue;
		touch[m].slot = touch[i].slot;
		m++;
	}
	for (i = 0; i < m; i++)
		touch[i].image = slots[touch[i].slot];
	*st = e.st;
	*ntouch = m;
	return 0;
}
