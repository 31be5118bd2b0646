/* Stand-alone churn of the NAT table's in-place arithmetic (mosrx_nat_apply,
 * csrc/nat_table.c) on a table for 1024 bindings: about 2 * 10^5 ADD and DEL ops
 * in calls of 1 .. 16 over 2048 candidate flows, the table rebuilt (emptied and
 * its live bindings added again, ids kept) whenever a call answers -ENOSPC.
 * After every call a walk written here -- from the key's hash, at most `probe`
 * slots, a free slot ends it, a delete marker is stepped over -- must find both
 * keys of every live binding with their kind, value and id, and neither key of
 * every other candidate; the state's counts must be the table's; the touch list
 * must be ascending and, laid over the table as it was, give the table as it is.
 * Some calls are spoilt by one op that must be refused, and must leave every
 * byte alone.  Exit status 0 and a count on success.  Built plain and with
 * -fsanitize=address,undefined by tests/test_nat_update.py. */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mosrx_nat.h"

#define NCAND 2048u
#define NLIVE 900u           /* live at most: room for some hundred tombstones between rebuilds */
#define NSLOTS 4096u          /* mosrx_nat_slots(1024) */
#define MAXOPS 16u
#define TOTAL 200000u

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 16);
}

static mosrx_nat_binding cand[NCAND];
static uint32_t hc[NCAND], hs[NCAND];      /* the hashes of a candidate's two keys */
static int live[NCAND];
static uint32_t id_of[NCAND];
static mosrx_nat_slot table[NSLOTS], before[NSLOTS];
static mosrx_nat_touch touch[4 * NCAND];
static mosrx_nat_tstate st;

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)

static uint16_t swap16(uint32_t v) { return (uint16_t)((v & 0xFFu) << 8 | (v >> 8 & 0xFFu)); }

/* The slot of the live key, -1: none. */
static int64_t walk(uint32_t h, uint32_t sa, uint32_t da, uint32_t pt)
{
	uint32_t d;
	for (d = 0; d < st.probe; d++) {
		const mosrx_nat_slot *s = &table[(h + d) & (NSLOTS - 1)];
		if (s->kind == 0)
			return -1;
		if (s->kind == MOSRX_NAT_TOMB)
			continue;
		if (s->kind != MOSRX_NAT_SNAT && s->kind != MOSRX_NAT_DNAT)
			FAIL("slot %u: kind %u", (h + d) & (NSLOTS - 1), s->kind);
		if (s->saddr == sa && s->daddr == da && s->ports == pt)
			return (int64_t)((h + d) & (NSLOTS - 1));
	}
	return -1;
}

static void check_all(uint32_t call)
{
	uint32_t i, keys = 0, tombs = 0, nlive = 0;
	for (i = 0; i < NSLOTS; i++) {
		const mosrx_nat_slot *s = &table[i];
		static const mosrx_nat_slot zero;
		mosrx_nat_slot t = zero;
		t.kind = MOSRX_NAT_TOMB;
		keys += s->kind == MOSRX_NAT_SNAT || s->kind == MOSRX_NAT_DNAT;
		tombs += s->kind == MOSRX_NAT_TOMB;
		if (s->kind == MOSRX_NAT_TOMB && memcmp(s, &t, sizeof(t)))
			FAIL("call %u: tombstone %u is not all zero", call, i);
		if (s->kind == 0 && memcmp(s, &zero, sizeof(zero)))
			FAIL("call %u: free slot %u is not all zero", call, i);
	}
	for (i = 0; i < NCAND; i++) {
		const mosrx_nat_binding *x = &cand[i];
		const int64_t a = walk(hc[i], x->cli_ip, x->svr_ip, (uint32_t)x->cli_port | (uint32_t)x->svr_port << 16);
		const int64_t b = walk(hs[i], x->svr_ip, x->nat_ip, (uint32_t)x->svr_port | (uint32_t)x->nat_port << 16);
		if (!live[i]) {
			if (a >= 0 || b >= 0)
				FAIL("call %u: candidate %u is not bound, yet found", call, i);
			continue;
		}
		nlive++;
		if (a < 0 || b < 0)
			FAIL("call %u: live binding %u not found within probe %u", call, i, st.probe);
		if (table[a].kind != MOSRX_NAT_SNAT || table[a].addr != x->nat_ip || table[a].port != x->nat_port ||
		    table[a].bind != id_of[i] || table[b].kind != MOSRX_NAT_DNAT || table[b].addr != x->cli_ip ||
		    table[b].port != x->cli_port || table[b].bind != id_of[i])
			FAIL("call %u: live binding %u: wrong value", call, i);
	}
	if (st.slots != NSLOTS || st.keys != keys || st.tombs != tombs || keys != 2 * nlive || keys + tombs > NSLOTS / 2)
		FAIL("call %u: state {%u %u %u %u}, table keys %u tombs %u, live %u", call, st.slots, st.keys, st.tombs, st.probe,
		     keys, tombs, nlive);
}

static void check_touch(uint32_t call, uint32_t m)
{
	uint32_t i;
	for (i = 0; i < m; i++) {
		if (touch[i].slot >= NSLOTS || (i && touch[i].slot <= touch[i - 1].slot))
			FAIL("call %u: touch %u: slot %u", call, i, touch[i].slot);
		before[touch[i].slot] = touch[i].image;
	}
	if (memcmp(before, table, sizeof(table)))
		FAIL("call %u: the touch list over the old table is not the new table", call);
}

/* Empty the table and add the live bindings again under their ids. */
static void rebuild(void)
{
	static mosrx_nat_op ops[NCAND];
	uint32_t i, n = 0, m;
	int rc;
	memset(table, 0, sizeof(table));
	st.slots = NSLOTS;
	st.keys = st.tombs = st.probe = 0;
	for (i = 0; i < NCAND; i++)
		if (live[i]) {
			ops[n].b = cand[i];
			ops[n].op = MOSRX_NAT_OP_ADD;
			ops[n].bind = id_of[i];
			n++;
		}
	if ((rc = mosrx_nat_apply(table, &st, ops, n, touch, &m)) || m != 2 * n)
		FAIL("rebuild of %u bindings: %d, %u slots touched", n, rc, m);
}

int main(void)
{
	uint32_t i, done = 0, call = 0, nlive = 0, rebuilds = 0, refused = 0, next_id = 1;
	for (i = 0; i < NCAND; i++) {
		mosrx_nat_binding *x = &cand[i];
		x->cli_ip = 10u | (i % 250u + 1u) << 24 | (i / 250u) << 16;
		x->svr_ip = 198u | 51u << 8 | 100u << 16 | (7u + i % 3u) << 24;
		x->nat_ip = 192u | 2u << 16 | 1u << 24;
		x->cli_port = swap16(20000u + i * 7u % 30000u);
		x->svr_port = swap16(i % 2u ? 80u : 443u);
		x->nat_port = swap16(1025u + i);
		hc[i] = mosrx_nat_hash_key(x->cli_ip, x->svr_ip, (uint32_t)x->cli_port | (uint32_t)x->svr_port << 16);
		hs[i] = mosrx_nat_hash_key(x->svr_ip, x->nat_ip, (uint32_t)x->svr_port | (uint32_t)x->nat_port << 16);
	}
	rebuild();
	check_all(0);
	while (done < TOTAL) {
		mosrx_nat_op ops[MAXOPS];
		uint32_t pick[MAXOPS], n = 1u + rnd() % MAXOPS, k, j, m = 0, spoil = MAXOPS, was_live = nlive;
		mosrx_nat_tstate st0 = st;
		int rc, want = 0, again;
		call++;
		/* distinct candidates: a live one is deleted, another added under a fresh id */
		for (k = 0; k < n; k++) {
			do {
				pick[k] = rnd() % NCAND;
				for (j = 0; j < k && pick[j] != pick[k]; j++)
					;
			} while (j < k || (!live[pick[k]] && nlive >= NLIVE));
			ops[k].b = cand[pick[k]];
			ops[k].op = live[pick[k]] ? MOSRX_NAT_OP_DEL : MOSRX_NAT_OP_ADD;
			ops[k].bind = next_id + k;
			nlive += live[pick[k]] ? -1 : 1;
		}
		if (call % 9 == 0) {
			/* one op that must be refused, anywhere in the list */
			spoil = rnd() % n;
			switch (rnd() % 5) {
			case 0: ops[spoil].op = 3; want = -EINVAL; break;
			case 1: ops[spoil].b.nat_port = 0; want = -EINVAL; break;
			case 2: ops[spoil].op ^= 3u; want = ops[spoil].op == MOSRX_NAT_OP_ADD ? -EEXIST : -ENOENT; break;
			case 3:
				if (ops[spoil].op == MOSRX_NAT_OP_ADD) {
					ops[spoil].bind = MOSRX_NAT_NO_BIND;
					want = -EINVAL;
				} else {
					ops[spoil].b.nat_port ^= 0x100;   /* the binding named in full: another NAT port is not it */
					want = -ENOENT;
				}
				break;
			default: ops[spoil].b.nat_ip = 0; want = -EINVAL; break;
			}
		}
		for (again = 0;; again++) {
			memcpy(before, table, sizeof(table));
			rc = mosrx_nat_apply(table, &st, ops, n, touch, &m);
			if (rc != -ENOSPC || again)
				break;
			if (memcmp(before, table, sizeof(table)) || memcmp(&st0, &st, sizeof(st)))
				FAIL("call %u: -ENOSPC changed the table", call);
			rebuild();
			rebuilds++;
			st0 = st;
		}
		if (want) {
			/* (a spoilt call may also run out of room before the bad op is reached) */
			if (rc != want && rc != -ENOSPC)
				FAIL("call %u: spoilt op %u: %d, not %d", call, spoil, rc, want);
			if (memcmp(before, table, sizeof(table)) || memcmp(&st0, &st, sizeof(st)))
				FAIL("call %u: a refused call changed the table", call);
			nlive = was_live;
			refused++;
			check_all(call);
			continue;
		}
		if (rc)
			FAIL("call %u: %d", call, rc);
		for (k = 0; k < n; k++) {
			live[pick[k]] = !live[pick[k]];
			id_of[pick[k]] = ops[k].bind;
		}
		next_id += n;
		done += n;
		if (st.probe < st0.probe)
			FAIL("call %u: probe shrank from %u to %u", call, st0.probe, st.probe);
		check_touch(call, m);
		check_all(call);
	}
	if (!rebuilds || !refused)
		FAIL("%u rebuilds, %u refused calls: the churn did not reach them", rebuilds, refused);
	printf("checked %u ops in %u calls, %u rebuilds, %u refused calls, %u live, probe %u\n", done, call, rebuilds, refused,
	       nlive, st.probe);
	return 0;
}
