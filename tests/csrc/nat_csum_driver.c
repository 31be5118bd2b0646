/* Stand-alone check of csrc/mosrx_nat.h's arithmetic against the oracle's full
 * recompute (oracle/mosrx_oracle.c: mo_ip_fast_csum, mo_tcp_csum), on random
 * valid frames: ihl 5..15, odd and even segment lengths, received check words of
 * 0x0000 and 0xFFFF, and rewrites chosen so that the new sum's residue is 0 and
 * so that the new check is 0xFFFE and 0x0001.  Exact equality on every frame;
 * exit status 0 and a count on success.  Built plain and with
 * -fsanitize=address,undefined by tests/test_nat.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mosrx_nat.h"
#include "mosrx_oracle.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
	rng_state ^= rng_state << 13;
	rng_state ^= rng_state >> 7;
	rng_state ^= rng_state << 17;
	return (uint32_t)(rng_state >> 16);
}

static uint32_t ld32(const uint8_t *p)
{
	uint32_t v;
	memcpy(&v, p, 4);
	return v;
}

static uint16_t ld16(const uint8_t *p)
{
	uint16_t v;
	memcpy(&v, p, 2);
	return v;
}

/* The IPv4 packet (no Ethernet header) of one valid TCP segment. */
static uint32_t make_packet(uint8_t *pk, uint32_t ihl, uint32_t seg)
{
	const uint32_t ip_len = 4 * ihl + seg;
	uint32_t i;
	uint16_t v;
	for (i = 0; i < ip_len + 4; i++)
		pk[i] = (uint8_t)rnd();
	pk[0] = (uint8_t)(0x40 | ihl);
	pk[2] = (uint8_t)(ip_len >> 8);
	pk[3] = (uint8_t)ip_len;
	pk[9] = 6;
	pk[10] = pk[11] = 0;
	v = mo_ip_fast_csum(pk, ihl);
	memcpy(pk + 10, &v, 2);
	pk[4 * ihl + 12] = (uint8_t)(0x50 | (pk[4 * ihl + 12] & 0xF));   /* doff 5 */
	pk[4 * ihl + 16] = pk[4 * ihl + 17] = 0;
	v = mo_tcp_csum(pk + 4 * ihl, (uint16_t)seg, ld32(pk + 12), ld32(pk + 16));
	memcpy(pk + 4 * ihl + 16, &v, 2);
	return ip_len;
}

/* The received packet must verify: the sum with its check word in place is 0. */
static int verifies(const uint8_t *pk, uint32_t ihl, uint32_t seg)
{
	return mo_tcp_csum(pk + 4 * ihl, (uint16_t)seg, ld32(pk + 12), ld32(pk + 16)) == 0;
}

static unsigned long checked, zero_residue, c_ffff, c_0000, new_fffe, new_0001;

/* One rewrite of pk, checked both ways; returns 0 on equality. */
static int check_one(const uint8_t *pk, uint32_t ihl, uint32_t seg, uint32_t kind, uint32_t addr, uint16_t port)
{
	uint8_t tr[15 * 4 + 1600 + 8];
	const uint32_t ip_len = 4 * ihl + seg, th = 4 * ihl;
	const int snat = kind == MOSRX_NAT_SNAT;
	const uint32_t a_old = ld32(pk + (snat ? 12 : 16));
	const uint16_t p_old = ld16(pk + th + (snat ? 0 : 2)), c_old = ld16(pk + th + 16);
	uint16_t want_ip, want_tcp, got_ip, got_tcp;
	uint64_t acc = 0;
	uint32_t j;
	/* the oracle: the sample's two overwrites, both checks recomputed in full */
	memcpy(tr, pk, ip_len + 4);
	memcpy(tr + (snat ? 12 : 16), &addr, 4);
	memcpy(tr + th + (snat ? 0 : 2), &port, 2);
	tr[10] = tr[11] = 0;
	want_ip = mo_ip_fast_csum(tr, ihl);
	tr[th + 16] = tr[th + 17] = 0;
	want_tcp = mo_tcp_csum(tr + th, (uint16_t)seg, ld32(tr + 12), ld32(tr + 16));
	/* the code under test: the received header's dwords and the received check word alone */
	for (j = 0; j < ihl; j++)
		acc = mosrx_nat_ip_acc(acc, mosrx_nat_ip_word(j, ld32(pk + 4 * j), kind, addr));
	got_ip = mosrx_nat_ip_fold(acc);
	got_tcp = mosrx_nat_tcp_check(a_old, addr, p_old, port, c_old);
	checked++;
	zero_residue += want_tcp == 0;
	c_ffff += c_old == 0xFFFF;
	c_0000 += c_old == 0;
	new_fffe += want_tcp == 0xFFFE;
	new_0001 += want_tcp == 0x0001;
	if (got_ip != want_ip || got_tcp != want_tcp) {
		fprintf(stderr, "ihl %u seg %u kind %u addr %08x port %04x c_old %04x: ip %04x want %04x, tcp %04x want %04x\n",
		        ihl, seg, kind, addr, port, c_old, got_ip, want_ip, got_tcp, want_tcp);
		return 1;
	}
	return 0;
}

/* The port that makes the rewritten segment's check word `target`, the address
 * given: the check is linear in the port modulo 0xFFFF. */
static uint16_t port_for(const uint8_t *pk, uint32_t ihl, uint32_t seg, uint32_t kind, uint32_t addr, uint16_t target)
{
	uint8_t tr[15 * 4 + 1600 + 8];
	const uint32_t th = 4 * ihl;
	const int snat = kind == MOSRX_NAT_SNAT;
	uint16_t zero = 0, c0;
	uint32_t f0, ft, p;
	memcpy(tr, pk, 4 * ihl + seg + 4);
	memcpy(tr + (snat ? 12 : 16), &addr, 4);
	memcpy(tr + th + (snat ? 0 : 2), &zero, 2);
	tr[th + 16] = tr[th + 17] = 0;
	c0 = mo_tcp_csum(tr + th, (uint16_t)seg, ld32(tr + 12), ld32(tr + 16));
	f0 = 0xFFFFu - c0;          /* the folded sum with port 0: 1 .. 0xFFFF */
	ft = 0xFFFFu - target;      /* the folded sum wanted */
	p = (ft + 0xFFFFu - f0) % 0xFFFFu;
	return (uint16_t)p;
}

int main(void)
{
	static uint8_t pk[15 * 4 + 1600 + 8];
	uint32_t it, ihl, fails = 0;
	for (it = 0; it < 60000 && !fails; it++) {
		const uint32_t seg = 20 + rnd() % 1200, kind = it & 1 ? MOSRX_NAT_SNAT : MOSRX_NAT_DNAT;
		uint32_t addr = rnd() | 1u;
		uint16_t port;
		ihl = 5 + it % 11;
		make_packet(pk, ihl, seg);
		if (it % 7 == 3 || it % 7 == 4) {
			/* a received check word of 0x0000: steer the source port so the rest sums to residue 0; 0xFFFF is the
			 * same residue, and a sender may store either */
			uint16_t p = port_for(pk, ihl, seg, MOSRX_NAT_SNAT, ld32(pk + 12), 0), v;
			memcpy(pk + 4 * ihl, &p, 2);
			pk[4 * ihl + 16] = pk[4 * ihl + 17] = 0;
			v = mo_tcp_csum(pk + 4 * ihl, (uint16_t)seg, ld32(pk + 12), ld32(pk + 16));
			if (it % 7 == 4 && v == 0)
				v = 0xFFFF;
			memcpy(pk + 4 * ihl + 16, &v, 2);
		}
		if (!verifies(pk, ihl, seg)) {
			fprintf(stderr, "generator: frame %u does not verify\n", it);
			return 2;
		}
		port = (uint16_t)rnd();
		if (it % 5 == 0)
			port = port_for(pk, ihl, seg, kind, addr, 0x0000);   /* the new sum's residue 0 */
		else if (it % 5 == 1)
			port = port_for(pk, ihl, seg, kind, addr, 0xFFFE);
		else if (it % 5 == 2)
			port = port_for(pk, ihl, seg, kind, addr, 0x0001);
		fails += check_one(pk, ihl, seg, kind, addr, port);
	}
	if (fails)
		return 1;
	printf("checked %lu zero_residue %lu c_old_ffff %lu c_old_0000 %lu new_fffe %lu new_0001 %lu\n", checked, zero_residue,
	       c_ffff, c_0000, new_fffe, new_0001);
	return !(zero_residue > 1000 && c_ffff > 1000 && c_0000 > 1000 && new_fffe > 1000 && new_0001 > 1000);
}
