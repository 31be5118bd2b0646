/*
 * mosrx_nat.h — shared between the C host library (nat_api.c, nat_table.c), the
 * NAT kernels (mosrx_nat.hip) and the stand-alone drivers (tests/csrc/nat_csum_driver.c,
 * tests/csrc/nat_update_driver.c).
 * Plain C layout; the arithmetic below compiles for the host and the device.
 */
#ifndef MOSRX_NAT_H
#define MOSRX_NAT_H

#include "mosrx_fwd.h"

#ifdef __HIPCC__
#define MOSRX_NAT_HD __host__ __device__ static inline
#else
#define MOSRX_NAT_HD static inline
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* One lane per frame (plan-nat) or per entry (patch); the tile is the forwarding
 * launches', so a queue's tile_base[] (mosrx_fdesc) serves both. */
#define MOSRX_NAT_THREADS 256u
#define MOSRX_NAT_TILE    MOSRX_FWD_TILE
#define MOSRX_NAT_MIN_SLOTS 16u

/* ---- the arithmetic --------------------------------------------------------------- */
/* Every value is the raw load of a little-endian host from network-order bytes,
 * as mOS's own sums take them (ip_fast_csum, TCPCalcChecksum): one's-complement
 * sums do not care, as long as every word is taken the same way. */

/* The slot hash of a key: (saddr, daddr, sport | dport << 16). */
MOSRX_NAT_HD uint32_t mosrx_nat_hash_key(uint32_t saddr, uint32_t daddr, uint32_t ports)
{
	uint32_t h = saddr * 0x9E3779B1u;
	h ^= (daddr * 0x85EBCA6Bu) << 13 | (daddr * 0x85EBCA6Bu) >> 19;
	h ^= ports * 0xC2B2AE35u;
	h ^= h >> 15;
	h *= 0x2C1B3C6Du;
	h ^= h >> 12;
	h *= 0x297A2D39u;
	h ^= h >> 15;
	return h;
}

/* Dword j of the IPv4 header as the translated header holds it: the check field
 * (the high half of dword 2) zero, saddr (dword 3, SNAT) or daddr (dword 4, DNAT)
 * the new address. */
MOSRX_NAT_HD uint32_t mosrx_nat_ip_word(uint32_t j, uint32_t w, uint32_t kind, uint32_t addr)
{
	if (j == 2u)
		return w & 0xFFFFu;
	if ((j == 3u && kind == MOSRX_NAT_SNAT) || (j == 4u && kind == MOSRX_NAT_DNAT))
		return addr;
	return w;
}

/* ip_fast_csum over ihl dwords added into acc one by one (acc from 0; at most 15
 * dwords: no overflow), then folded: the value mOS stores in iph->check. */
MOSRX_NAT_HD uint64_t mosrx_nat_ip_acc(uint64_t acc, uint32_t w)
{
	return acc + w;
}

MOSRX_NAT_HD uint16_t mosrx_nat_ip_fold(uint64_t acc)
{
	/* 2^16 is 1 modulo 0xFFFF: the four halves add; a sum that is not 0 folds to 1 .. 0xFFFF as the carries of
	 * ip_fast_csum leave it (the version nibble keeps the header's sum from 0) */
	uint32_t s = (uint32_t)(acc & 0xFFFFu) + (uint32_t)((acc >> 16) & 0xFFFFu) + (uint32_t)((acc >> 32) & 0xFFFFu) +
	             (uint32_t)(acc >> 48);
	s = (s & 0xFFFFu) + (s >> 16);
	s = (s & 0xFFFFu) + (s >> 16);
	return (uint16_t)~s;
}

/* tcph->check after the rewrite, from the received check word alone.  TCP_OK
 * means the received segment and pseudo header sum to 0 modulo 0xFFFF, check
 * word included; so the sum TCPCalcChecksum takes over the rewritten segment
 * with its check word zeroed is congruent to A_new - A_old - C_old, A the sum
 * of the address and port words that change.  Its double fold leaves the
 * representative in 1 .. 0xFFFF (the sum is never 0: the protocol word is not),
 * residue 0 as 0xFFFF, and the check is its complement. */
MOSRX_NAT_HD uint16_t mosrx_nat_tcp_check(uint32_t a_old, uint32_t a_new, uint32_t p_old, uint32_t p_new, uint32_t c_old)
{
	const uint32_t an = (a_new & 0xFFFFu) + (a_new >> 16) + (p_new & 0xFFFFu);
	const uint32_t ao = (a_old & 0xFFFFu) + (a_old >> 16) + (p_old & 0xFFFFu) + (c_old & 0xFFFFu);
	/* ao <= 4 * 0xFFFF: five times 0xFFFF on top keeps x in 0xFFFF .. 8 * 0xFFFF, positive and the same residue */
	uint32_t x = an + 5u * 0xFFFFu - ao;
	x = (x & 0xFFFFu) + (x >> 16);
	x = (x & 0xFFFFu) + (x >> 16);   /* 1 .. 0xFFFF */
	return (uint16_t)(0xFFFFu - x);
}

/* ---- the launches ------------------------------------------------------------------ */

/* plan-nat: the plan launch's own parameters (one batch: f whole; the queue form:
 * f's tab / forward / num_msp / listener, the batches from fdesc), the table and
 * the xlat outputs. */
typedef struct mosrx_nparams {
	mosrx_fparams f;
	const mosrx_nat_slot *slots;   /* mask + 1 of them */
	uint32_t mask, probe;          /* probe: the most slots a lookup examines (0: an empty table) */
	mosrx_nat_xlat *xlat;          /* the single batch: n, 16-byte aligned */
	/* the queue form (fdesc != NULL): nb batches, device-resident; xtab[k] batch k's xlat array */
	const mosrx_fdesc *fdesc;
	mosrx_nat_xlat *const *xtab;
	uint32_t nb, total_tiles;
} mosrx_nparams;

/* patch: the ring build's outputs of one batch, or the queue's fdesc table. */
typedef struct mosrx_npatch {
	const mosrx_nat_xlat *xlat;
	uint8_t *tx;
	const uint32_t *tx_off, *tx_src;
	const mosrx_fwd_ring *rings;
	uint32_t nrings, n;
	const mosrx_fdesc *fdesc;
	mosrx_nat_xlat *const *xtab;
	uint32_t nb, total_tiles;
} mosrx_npatch;

/* One launch each on `stream`; 0, -EINVAL or -EIO.  Allocate nothing.  Nothing to
 * do (n == 0, a queue of empty batches) launches nothing. */
int mosrx_launch_nat_plan(const mosrx_nparams *np, void *stream);
int mosrx_launch_nat_patch(const mosrx_npatch *pp, void *stream);
/* update: lane i of ceil(m / 256) workgroups stores touch[i].image into
 * slots[touch[i].slot] when that slot is <= mask, as two 16-byte stores; the
 * host made the slots distinct (mosrx_nat_apply), so no two lanes meet.  touch
 * may be pinned host memory, by its device address.  -EINVAL, before any launch,
 * for a NULL or misaligned (16) table or touch array and for a mask that is not
 * 2^k - 1 or is below MOSRX_NAT_MIN_SLOTS - 1. */
int mosrx_launch_nat_update(mosrx_nat_slot *slots, uint32_t mask, const mosrx_nat_touch *touch, uint32_t m, void *stream);

/* ---- the table's arithmetic (nat_table.c), as nat_api.c reaches it ------------------- */
/* mosrx_nat_build with binding i's id ids[i] (NULL: i), into a table of cap slots
 * (0: mosrx_nat_slots(n), and no fewer; a power of two). */
int mosrx__nat_build_ids(const mosrx_nat_binding *b, const uint32_t *ids, uint32_t n, mosrx_nat_slot *slots, uint32_t cap,
                         uint32_t *probe);
/* The live bindings of a table and their ids, in slot order of their client-side
 * keys, into b[max] / ids[max]; returns how many there are (more than max: only
 * max were written). */
uint32_t mosrx__nat_live(const mosrx_nat_slot *slots, uint32_t nslots, mosrx_nat_binding *b, uint32_t *ids, uint32_t max);

#ifdef __cplusplus
}
#endif
#endif
