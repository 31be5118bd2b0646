// mosrx_fwd.hip — forwarding for forward = 1 stacks: what ProcessPacket does
// with a frame it passes on, over a classified batch.
//
//   plan   one lane per frame: mosrx_mos_forwards' rule on the record's reason,
//          then ForwardEthernetFrame (eth_out.c:104-134) or ForwardIPPacket
//          (ip_out.c:39-110) up to the point where mOS asks for a TX buffer:
//          the nic_forward_table entry, else GetOutputInterface's walk
//          (ip_out.c:11-37) and GetDestinationHWaddr's (arp.c:88-119), both
//          over tables held in LDS (every lane reads the same entry per step:
//          a broadcast read).  One 8-byte mosrx_fwd per frame, one store.
//   build  three ordinary launches over tiles of MOSRX_FWD_TILE frames:
//     1. totals  per tile: 16-byte TX units and sent frames (from the plan)
//     2. scan    one workgroup: exclusive prefix over the tiles' totals (each
//                tile's base overwrites its row), tx_count = {0, 0}
//     3. copy    per tile: the same per-frame units scanned inside the tile,
//                tx_off / tx_len / tx_nif / tx_src stored, then the tile's TX
//                units dealt round robin over the lanes -- lane-adjacent units
//                are adjacent 16-byte stores -- each unit finding its frame by
//                binary search of the tile's unit starts in LDS.
// No workgroup waits on another within a launch; every loop's bound is known
// at its entry; every store is guarded by the frame fitting tx_cap (units are
// recomputed from the plan in the copy launch itself, so a plan that changes
// under the launches cannot move a store out of tx_frames) and j < n.
//
// Sent frame j starts at 16 k + 2: its 14-byte header fills bytes 2..15 of its
// first unit (one short + three dword stores), and unit r >= 1 holds frame
// bytes 16 r - 2 .. 16 r + 13, read from any source alignment as five aligned
// dwords through the batch's buffer resource and realigned with v_alignbyte;
// one dwordx4 store, partial dwords / bytes only in a frame's last unit.
// Padding between frames is never written.
//
// The plan and the ring build also run over a whole batch queue
// (mosrx_launch_fwd_queue): the same bodies, a workgroup finding its batch in a
// device-resident table first, four launches whatever the number of batches.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "mosrx_device.h"
#include "mosrx_fwd.h"

#define FWD_SCAN_THREADS 1024u
#define FWD_WAVES (MOSRX_FWD_THREADS / 64u)

static_assert(sizeof(mosrx_fwd) == 8 && MOSRX_FWD_ROW == 16u, "8-byte plan records, 16-byte scratch rows");
static_assert(MOSRX_FWD_TILE == MOSRX_FWD_THREADS && MOSRX_FWD_TILE == 256u, "one lane per frame; 8 search steps");

// bytes a .. a+3 of the batch buffer, any alignment (zero past its end)
__device__ __forceinline__ uint32_t fwd_ld32(__amdgpu_buffer_rsrc_t r, uint32_t a)
{
	const uint32_t a4 = a & ~3u;
	const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(r, a4, 0, 0);
	const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(r, a4 + 4u, 0, 0);
	return __builtin_amdgcn_alignbyte(hi, lo, a & 3u);
}

// bytes a .. a+15
__device__ __forceinline__ u32x4 fwd_ld128(__amdgpu_buffer_rsrc_t r, uint32_t a)
{
	const uint32_t a4 = a & ~3u, sh = a & 3u;
	const u32x4 q = __builtin_amdgcn_raw_buffer_load_b128(r, a4, 0, 0);
	const uint32_t e = __builtin_amdgcn_raw_buffer_load_b32(r, a4 + 16u, 0, 0);
	u32x4 v;
	v.x = __builtin_amdgcn_alignbyte(q.y, q.x, sh);
	v.y = __builtin_amdgcn_alignbyte(q.z, q.y, sh);
	v.z = __builtin_amdgcn_alignbyte(q.w, q.z, sh);
	v.w = __builtin_amdgcn_alignbyte(e, q.w, sh);
	return v;
}

// ---- plan ------------------------------------------------------------------
// Workgroup `blk` of the batch in p (both plan kernels' body): frames blk * 256 ..
template <uint32_t RB>
__device__ __forceinline__ void fwd_plan_body(const mosrx_fparams p, uint32_t blk)
{
	__shared__ uint32_t s_rm[MOSRX_FWD_MAX_ROUTES], s_rv[MOSRX_FWD_MAX_ROUTES];
	__shared__ int32_t s_rp[MOSRX_FWD_MAX_ROUTES], s_rn[MOSRX_FWD_MAX_ROUTES];
	__shared__ uint32_t s_am[MOSRX_FWD_MAX_ARP], s_av[MOSRX_FWD_MAX_ARP];
	__shared__ int32_t s_ap[MOSRX_FWD_MAX_ARP];
	const uint32_t t = threadIdx.x, i = blk * MOSRX_FWD_THREADS + t;
#define FWD_PLAN 1
#include "mosrx_fwd_plan_body.inc"
	if (i >= p.n)
		return;
#define FWD_PLAN 2
#include "mosrx_fwd_plan_body.inc"
	*reinterpret_cast<u32x2 *>(p.plan + i) = v;
}

template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_plan_kernel(mosrx_fparams p)
{
	fwd_plan_body<RB>(p, blockIdx.x);
}

// ---- the batch-queue form ----------------------------------------------------
// The batch of tile `blk` of a queue launch: find k with tile_base[k] <= blk <
// tile_base[k+1], as the steer queue form does (empty batches share their
// successor's base and are skipped).  The bound is known at entry and the
// search is uniform over the workgroup.
__device__ __forceinline__ mosrx_fdesc fwd_queue_batch(const mosrx_fqparams &fq, uint32_t blk)
{
	uint32_t lo = 0, hi = fq.nb;
	for (int it = 0; it < 32 && hi - lo > 1; it++) {
		const uint32_t mid = (lo + hi) >> 1;
		if (fq.desc[mid].tile_base <= blk)
			lo = mid;
		else
			hi = mid;
	}
	return fq.desc[lo];
}

// Plan over every batch of a queue: the nic_fwd[in_ifidx] shortcut (and with
// it the LDS table copy) is decided per workgroup from its batch's in_ifidx.
template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_plan_queue_kernel(mosrx_fqparams fq)
{
	if (blockIdx.x >= fq.total_tiles)
		return;
	const mosrx_fdesc d = fwd_queue_batch(fq, blockIdx.x);
	mosrx_fparams p = {};
	p.frames = d.frames;
	p.off = d.off;
	p.len = d.len;
	p.rec = d.rec;
	p.tab = fq.tab;
	p.plan = d.plan;
	p.frames_bytes = d.frames_bytes;
	p.n = d.n;
	p.in_ifidx = (int32_t)d.in_ifidx;
	p.forward = fq.forward;
	p.num_msp = fq.num_msp;
	p.listener = fq.listener;
	fwd_plan_body<RB>(p, blockIdx.x - d.tile_base);
}

// ---- build -----------------------------------------------------------------
// A plan record's share of the TX run: sent (kind IP or ETH with a whole
// Ethernet header) and its 16-byte units, ceil((2 + tx_len) / 16).
__device__ __forceinline__ uint32_t fwd_units(u32x2 pl)
{
	const uint32_t kind = pl.x >> 24, tx_len = pl.x & 0xFFFFu;
	const bool sent = (kind == MOSRX_FWD_IP || kind == MOSRX_FWD_ETH) && tx_len >= 14u;
	return sent ? (tx_len + 2u + 15u) >> 4 : 0u;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
	for (uint32_t o = 1; o < 64u; o <<= 1) {
		const uint32_t x = __shfl_up(v, o);
		v += lane >= o ? x : 0u;
	}
	return v;
}

// The tile's frames: this lane's exclusive unit offset and sent rank inside
// the tile; tot_units / tot_sent the tile's totals (the same in every lane).
__device__ __forceinline__ void fwd_tile_scan(uint32_t units, uint32_t *s_wu, uint32_t *s_wc, uint32_t &excl,
                                              uint32_t &rank, uint32_t &tot_units, uint32_t &tot_sent)
{
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	const uint32_t inc = wave_incl_scan(units, lane);
	const uint64_t sm = __ballot(units != 0u);
	const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(sm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sm, 0u));
	if (lane == 63u) {
		s_wu[wave] = inc;
		s_wc[wave] = (uint32_t)__builtin_popcountll(sm);
	}
	__syncthreads();
	uint32_t bu = 0, bc = 0;
	tot_units = tot_sent = 0;
#pragma unroll
	for (uint32_t w = 0; w < FWD_WAVES; w++) {
		const uint32_t u = s_wu[w], c = s_wc[w];
		bu += w < wave ? u : 0u;
		bc += w < wave ? c : 0u;
		tot_units += u;
		tot_sent += c;
	}
	excl = bu + inc - units;
	rank = bc + below;
}

// 1. totals: scratch row = {units, sent, 0, 0}
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_totals_kernel(mosrx_fparams p)
{
	__shared__ uint32_t s_wu[FWD_WAVES], s_wc[FWD_WAVES];
	if (blockIdx.x >= p.tiles)
		return;
	const uint32_t t = threadIdx.x, i = blockIdx.x * MOSRX_FWD_TILE + t;
	u32x2 pl = {0u, 0u};
	if (i < p.n)
		pl = *reinterpret_cast<const u32x2 *>(p.plan + i);
	uint32_t excl, rank, tu, ts;
	fwd_tile_scan(fwd_units(pl), s_wu, s_wc, excl, rank, tu, ts);
	if (t == 0) {
		u32x4 row = {tu, ts, 0u, 0u};
		*reinterpret_cast<u32x4 *>(p.scratch + 4u * blockIdx.x) = row;
	}
}

// 2. scan: lane t owns a run of `per` consecutive tiles; rows become
//    {unit base lo, unit base hi, sent base, 0}
__global__ __launch_bounds__(FWD_SCAN_THREADS) void mosrx_fwd_scan_kernel(mosrx_fparams p)
{
	__shared__ uint64_t s_u[FWD_SCAN_THREADS];
	__shared__ uint32_t s_c[FWD_SCAN_THREADS];
	const uint32_t t = threadIdx.x;
	if (blockIdx.x != 0)
		return;
	const uint32_t per = (p.tiles + FWD_SCAN_THREADS - 1u) / FWD_SCAN_THREADS;
	const uint32_t t0 = min(t * per, p.tiles), t1 = min(t0 + per, p.tiles);
	uint64_t su = 0;
	uint32_t sc = 0;
	for (uint32_t r = t0; r < t1; r++) {
		su += p.scratch[4u * r];
		sc += p.scratch[4u * r + 1u];
	}
	s_u[t] = su;
	s_c[t] = sc;
	__syncthreads();
	// inclusive prefix over the 1024 runs (Hillis-Steele, 10 steps)
#pragma unroll
	for (uint32_t o = 1; o < FWD_SCAN_THREADS; o <<= 1) {
		const uint64_t vu = t >= o ? s_u[t - o] : 0u;
		const uint32_t vc = t >= o ? s_c[t - o] : 0u;
		__syncthreads();
		s_u[t] += vu;
		s_c[t] += vc;
		__syncthreads();
	}
	uint64_t ru = s_u[t] - su;
	uint32_t rc = s_c[t] - sc;
	for (uint32_t r = t0; r < t1; r++) {
		const uint32_t u = p.scratch[4u * r], c = p.scratch[4u * r + 1u];
		u32x4 row = {(uint32_t)ru, (uint32_t)(ru >> 32), rc, 0u};
		*reinterpret_cast<u32x4 *>(p.scratch + 4u * r) = row;
		ru += u;
		rc += c;
	}
	if (t == 0) {
		p.tx_count[0] = 0;
		p.tx_count[1] = 0;
	}
}

// 3. copy
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_copy_kernel(mosrx_fparams p)
{
	__shared__ uint32_t s_wu[FWD_WAVES], s_wc[FWD_WAVES];
	__shared__ uint32_t s_start[MOSRX_FWD_TILE + 1u];   // unit start of the tile's k-th sent frame; [sent]: the tile's units
	__shared__ uint32_t s_off[MOSRX_FWD_TILE];          // its source offset
	__shared__ uint32_t s_meta[MOSRX_FWD_TILE];         // its plan word 0 (tx_len, out_ifidx, kind); 0: does not fit
	__shared__ uint32_t s_arp[MOSRX_FWD_TILE];
	if (blockIdx.x >= p.tiles)
		return;
	const uint32_t t = threadIdx.x, i = blockIdx.x * MOSRX_FWD_TILE + t;
	u32x2 pl = {0u, 0u};
	uint32_t o = 0;
	if (i < p.n) {
		pl = *reinterpret_cast<const u32x2 *>(p.plan + i);
		o = p.off[i];
	}
	const u32x4 row = *reinterpret_cast<const u32x4 *>(p.scratch + 4u * blockIdx.x);
	const uint64_t ubase = (uint64_t)row.x | ((uint64_t)row.y << 32);
	const uint32_t units = fwd_units(pl);
	uint32_t excl, rank, tu, ts;
	fwd_tile_scan(units, s_wu, s_wc, excl, rank, tu, ts);
	const bool sent = units != 0u;
	const uint64_t k = ubase + excl;
	const bool fits = sent && k + units <= (uint64_t)p.cap_units;
	const uint32_t j = row.z + rank;
	if (sent) {
		s_start[rank] = excl;
		s_off[rank] = o;
		s_meta[rank] = fits ? pl.x : 0u;
		s_arp[rank] = pl.y & 0xFFFFu;
	}
	if (t == 0)
		s_start[ts] = tu;
	if (fits && j < p.n) {
		p.tx_off[j] = (uint32_t)(k * 16u + 2u);
		p.tx_len[j] = (uint16_t)(pl.x & 0xFFFFu);
		p.tx_nif[j] = (int8_t)((pl.x >> 16) & 0xFFu);
		p.tx_src[j] = i;
	}
	{
		const uint32_t nfit = (uint32_t)__builtin_popcountll(__ballot(fits && j < p.n));
		const uint32_t ndrop = (uint32_t)__builtin_popcountll(__ballot(sent && !(fits && j < p.n)));
		if ((t & 63u) == 0u) {
			if (nfit)
				atomicAdd(&p.tx_count[0], nfit);
			if (ndrop)
				atomicAdd(&p.tx_count[1], ndrop);
		}
	}
	__syncthreads();
	const __amdgpu_buffer_rsrc_t rs = frame_rsrc(p.frames, p.frames_bytes);
	const mosrx_fwd_dev *T = p.tab;
	for (uint32_t u = t; u < tu; u += MOSRX_FWD_THREADS) {
		// the sent frame that holds unit u: the last one starting at or before it
		uint32_t lo = 0, hi = ts;
#pragma unroll
		for (int it = 0; it < 8; it++) {
			const uint32_t mid = (lo + hi) >> 1;
			const bool go = hi - lo > 1u;
			const bool le = s_start[mid] <= u;
			lo = go && le ? mid : lo;
			hi = go && !le ? mid : hi;
		}
		const uint32_t meta = s_meta[lo];
		if (!meta)
			continue;                      // the frame does not fit tx_cap
		const uint32_t r = u - s_start[lo];
		const uint32_t tx_len = meta & 0xFFFFu;
		const uint64_t ku = ubase + u;
		if (ku >= (uint64_t)p.cap_units)
			continue;                      // (holds by construction: the frame's last unit fits)
		uint8_t *dst = p.tx + ku * 16u;
		if (r == 0) {
			// the Ethernet header: EthernetOutput's rewrite for an IP frame, a copy otherwise
			u32x4 h = fwd_ld128(rs, s_off[lo]);
			if ((meta >> 24) == MOSRX_FWD_IP) {
				const uint32_t ai = s_arp[lo];
				const uint32_t nif = (meta >> 16) & (MOSRX_FWD_MAX_NETDEVS - 1u);
				const uint32_t *sm = reinterpret_cast<const uint32_t *>(T->netdev_haddr[nif]);
				const uint32_t s0 = sm[0], s1 = sm[1] & 0xFFFFu;
				uint32_t d0 = h.x, d1 = h.y & 0xFFFFu;   // the frame's own h_dest (nic_forward_table path)
				if (ai < MOSRX_FWD_MAX_ARP) {
					const uint32_t *dm = reinterpret_cast<const uint32_t *>(T->a_haddr[ai]);
					d0 = dm[0];
					d1 = dm[1] & 0xFFFFu;
				}
				h.x = d0;
				h.y = d1 | (s0 << 16);
				h.z = (s0 >> 16) | (s1 << 16);
			}
			*reinterpret_cast<uint16_t *>(dst + 2) = (uint16_t)h.x;
			*reinterpret_cast<uint32_t *>(dst + 4) = (h.x >> 16) | (h.y << 16);
			*reinterpret_cast<uint32_t *>(dst + 8) = (h.y >> 16) | (h.z << 16);
			*reinterpret_cast<uint32_t *>(dst + 12) = (h.z >> 16) | (h.w << 16);
		} else {
			const uint32_t b0 = 16u * r - 2u;      // the unit's first frame byte; < tx_len
			const uint32_t rem = tx_len - b0;
			const u32x4 v = fwd_ld128(rs, s_off[lo] + b0);
			if (rem >= 16u) {
				*reinterpret_cast<u32x4 *>(dst) = v;
			} else {
				const uint32_t w[4] = {v.x, v.y, v.z, v.w};
				const uint32_t nd = rem >> 2;
				uint32_t last = 0;
#pragma unroll
				for (uint32_t q = 0; q < 4u; q++) {
					if (q < nd)
						reinterpret_cast<uint32_t *>(dst)[q] = w[q];
					last = q == nd ? w[q] : last;
				}
				uint8_t *e = dst + 4u * nd;
				if (rem & 2u) {
					*reinterpret_cast<uint16_t *>(e) = (uint16_t)last;
					e += 2;
					last >>= 16;
				}
				if (rem & 1u)
					*e = (uint8_t)last;
			}
		}
	}
}

// ---- build, ring form ------------------------------------------------------
// The same three launches with one column per output netdev:
//   1. totals  per tile and netdev: units and sent frames, one scratch row of
//              nrings entries per tile
//   2. scan    one workgroup, wave q scanning netdev q's column over the tiles
//              (64-bit unit bases); rings[q] = {start, 0, 0, 0}, start the sent
//              frames of the netdevs below q, and folded into the column's
//              entry bases
//   3. copy    per tile: each frame's unit offset and rank among the frames of
//              its own netdev, its entry stored; then the tile's written
//              units dealt round robin over the lanes as in the arrival-order
//              copy, each unit finding its frame by binary search and its
//              destination through the frame's first ring unit in LDS
// The rank inside a tile is a masked scan per netdev: a loop of exactly nrings
// rounds, a round whose netdev no lane of the wave holds costing one ballot.
// (The steer kernels' ballot-per-key-bit mask gives a rank, not the sum of the
// units of the lanes below, which the offset needs.)  count / dropped are sums
// and units a maximum over the tiles, by atomics on what the scan zeroed: none
// depends on the order the workgroups run in.
static_assert(MOSRX_FWD_MAX_NETDEVS == 16 && sizeof(mosrx_fwd_ring) == 16, "ring rows");
#define FWD_NQ 16u

// A plan record's share of ring q = its out_ifidx: fwd_units' rule and q < nrings.
__device__ __forceinline__ uint32_t fwd_ring_units(u32x2 pl, uint32_t nrings, uint32_t &q)
{
	q = (pl.x >> 16) & 0xFFu;
	return q < nrings ? fwd_units(pl) : 0u;
}

// This lane's exclusive unit offset and rank among the tile's frames of its
// own netdev q (units != 0 only with q < nrings); s_wu / s_wc [wave][netdev]
// hold every wave's totals after it.
__device__ __forceinline__ void fwd_ring_tile_scan(uint32_t q, uint32_t units, uint32_t nrings,
                                                   uint32_t (*s_wu)[FWD_NQ], uint32_t (*s_wc)[FWD_NQ], uint32_t &excl,
                                                   uint32_t &rank)
{
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	uint32_t e = 0, r = 0;
	for (uint32_t g = 0; g < nrings; g++) {
		const bool mine = units != 0u && q == g;
		const uint64_t bm = __ballot(mine);
		uint32_t wu = 0;
		if (bm) {   // (uniform over the wave)
			const uint32_t inc = wave_incl_scan(mine ? units : 0u, lane);
			const uint32_t below =
				__builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u));
			e = mine ? inc - units : e;
			r = mine ? below : r;
			wu = inc;
		}
		if (lane == 63u) {
			s_wu[wave][g] = wu;
			s_wc[wave][g] = (uint32_t)__builtin_popcountll(bm);
		}
	}
	__syncthreads();
	const uint32_t qq = q & (FWD_NQ - 1u);
	uint32_t bu = 0, bc = 0;
#pragma unroll
	for (uint32_t w = 0; w < FWD_WAVES; w++) {
		bu += w < wave ? s_wu[w][qq] : 0u;
		bc += w < wave ? s_wc[w][qq] : 0u;
	}
	excl = bu + e;
	rank = bc + r;
}

// The ring build of a queue's batch as the single-batch bodies take it: the
// batch's own buffers, and its scratch rows from tile_base * nrings.
__device__ __forceinline__ mosrx_rparams fwd_queue_rparams(const mosrx_fqparams &fq, const mosrx_fdesc &d)
{
	mosrx_rparams p = {};
	p.frames = d.frames;
	p.off = d.off;
	p.tab = fq.tab;
	p.plan = d.plan;
	p.frames_bytes = d.frames_bytes;
	p.n = d.n;
	p.nrings = fq.nrings;
	p.cap_units = fq.cap_units;
	p.tiles = (d.n + MOSRX_FWD_TILE - 1u) / MOSRX_FWD_TILE;
	p.tx = d.tx;
	p.tx_off = d.tx_off;
	p.tx_len = d.tx_len;
	p.tx_src = d.tx_src;
	p.rings = d.rings;
	p.scratch = fq.scratch + 4u * ((uint64_t)d.tile_base * min(fq.nrings, FWD_NQ));
	return p;
}

// The three bodies are mosrx_fwd_rings_body.inc, shared with the queue forms.
// 1. totals: scratch row (tile, q) = {units, sent, 0, 0}
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_ring_totals_kernel(mosrx_rparams p)
{
#define FWD_BODY 1
#define FWD_BLK blockIdx.x
#include "mosrx_fwd_rings_body.inc"
}

__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_ring_totals_queue_kernel(mosrx_fqparams fq)
{
	if (blockIdx.x >= fq.total_tiles)
		return;
	const mosrx_fdesc d = fwd_queue_batch(fq, blockIdx.x);
	const mosrx_rparams p = fwd_queue_rparams(fq, d);
	// (the body's FWD_BLK < p.tiles holds by construction of tile_base[]: it keeps the row inside the batch's scratch)
#define FWD_BODY 1
#define FWD_BLK (blockIdx.x - d.tile_base)
#include "mosrx_fwd_rings_body.inc"
}

// 2. scan: wave q owns netdev q's column, lane l a run of `per` consecutive
//    tiles; rows become {unit base lo, unit base hi, rings[q].start + sent base, 0}
__global__ __launch_bounds__(FWD_SCAN_THREADS) void mosrx_fwd_ring_scan_kernel(mosrx_rparams p)
{
#define FWD_BODY 2
#define FWD_SKIP (blockIdx.x != 0)
#include "mosrx_fwd_rings_body.inc"
}

// One workgroup per batch of the queue; that of an empty batch only writes the zeroed rings.
__global__ __launch_bounds__(FWD_SCAN_THREADS) void mosrx_fwd_ring_scan_queue_kernel(mosrx_fqparams fq)
{
	if (blockIdx.x >= fq.nb)
		return;
	const mosrx_fdesc d = fq.desc[blockIdx.x];
	const mosrx_rparams p = fwd_queue_rparams(fq, d);
#define FWD_BODY 2
#define FWD_SKIP false
#include "mosrx_fwd_rings_body.inc"
}

// 3. copy
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_ring_copy_kernel(mosrx_rparams p)
{
#define FWD_BODY 3
#define FWD_BLK blockIdx.x
#include "mosrx_fwd_rings_body.inc"
}

__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_ring_copy_queue_kernel(mosrx_fqparams fq)
{
	if (blockIdx.x >= fq.total_tiles)
		return;
	const mosrx_fdesc d = fwd_queue_batch(fq, blockIdx.x);
	const mosrx_rparams p = fwd_queue_rparams(fq, d);
#define FWD_BODY 3
#define FWD_BLK (blockIdx.x - d.tile_base)
#include "mosrx_fwd_rings_body.inc"
}

// ---- build, descriptor ring form --------------------------------------------
// What a host that still holds the received frames lacks per sent frame: its
// netdev and place in it (the entry index), its source index, its TX length and
// the 12 address bytes EthernetOutput rewrites.  The ring form's totals and scan
// launches as they are (neither reads a capacity), then
//   3. store   per tile: the frame's rank among the tile's frames of its own
//              netdev (the same masked scan), its entry = the scan's entry base
//              + rank; tx_src / tx_len / the three tx_mac dwords stored by the
//              frame's own lane.  count and units are sums over the tiles, by
//              atomics on what the scan zeroed: neither depends on the order
//              the workgroups run in.
// Nothing is dropped, so units is the ring's whole need: what a byte ring
// large enough reports.
__device__ __forceinline__ void fwd_desc_store_body(const mosrx_dparams &p, uint32_t blk)
{
	__shared__ uint32_t s_wu[FWD_WAVES][FWD_NQ], s_wc[FWD_WAVES][FWD_NQ];
	// uniform over the workgroup (blk and p.tiles are the same in every lane): all
	// of its lanes leave here or all reach the barrier in fwd_ring_tile_scan
	if (blk >= p.tiles)
		return;
	const uint32_t nrings = min(p.nrings, FWD_NQ);
	const uint32_t t = threadIdx.x, i = blk * MOSRX_FWD_TILE + t;
	u32x2 pl = {0u, 0u};
	uint32_t o = 0;
	if (i < p.n) {
		pl = *reinterpret_cast<const u32x2 *>(p.plan + i);
		o = p.off[i];
	}
	uint32_t q, excl, rank;
	const uint32_t units = fwd_ring_units(pl, nrings, q);
	const bool sent = units != 0u;   // (then q < nrings and i < n)
	fwd_ring_tile_scan(q, units, nrings, s_wu, s_wc, excl, rank);
	uint32_t base = 0;
	if (sent)
		base = p.scratch[4u * ((uint64_t)blk * nrings + q) + 2u];
	const uint32_t j = base + rank;
	if (sent && j < p.n) {
#include "mosrx_fwd_desc_entry.inc"
	}
	if (t < nrings) {
		uint32_t tu = 0, tc = 0;
#pragma unroll
		for (uint32_t w = 0; w < FWD_WAVES; w++) {
			tu += s_wu[w][t];
			tc += s_wc[w][t];
		}
		mosrx_fwd_ring *rg = p.rings + t;
		if (tc) {
			atomicAdd(&rg->count, tc);
			atomicAdd(&rg->units, tu);
		}
	}
}

__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_desc_store_kernel(mosrx_dparams p)
{
	fwd_desc_store_body(p, blockIdx.x);
}

// The store launch over every batch of a queue: its own descriptor table, the
// same tile_base[] as the plan / totals launches', found the same way.
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_desc_store_queue_kernel(mosrx_dqparams dq)
{
	if (blockIdx.x >= dq.total_tiles)
		return;
	uint32_t lo = 0, hi = dq.nb;
	for (int it = 0; it < 32 && hi - lo > 1; it++) {
		const uint32_t mid = (lo + hi) >> 1;
		if (dq.desc[mid].tile_base <= blockIdx.x)
			lo = mid;
		else
			hi = mid;
	}
	const mosrx_ddesc d = dq.desc[lo];
	mosrx_dparams p = {};
	p.frames = d.frames;
	p.off = d.off;
	p.tab = dq.tab;
	p.plan = d.plan;
	p.frames_bytes = d.frames_bytes;
	p.n = d.n;
	p.nrings = dq.nrings;
	p.tiles = (d.n + MOSRX_FWD_TILE - 1u) / MOSRX_FWD_TILE;
	p.tx_src = d.tx_src;
	p.tx_len = d.tx_len;
	p.tx_mac = d.tx_mac;
	p.rings = d.rings;
	p.scratch = dq.scratch + 4u * ((uint64_t)d.tile_base * min(dq.nrings, FWD_NQ));
	fwd_desc_store_body(p, blockIdx.x - d.tile_base);
}

// ---- plan + descriptor rings, one launch --------------------------------------
// For batches of a tile or so the four launches above are launch latency and
// little else.  Here one workgroup owns a batch and walks it in tiles of
// MOSRX_FWD_TILE frames, lane t owning frame tile * 256 + t throughout:
//   1. per tile  the frame's plan record (PLAN: made as fwd_plan_body makes it
//                and stored; else loaded), its netdev, units and rank among the
//                tile's frames of that netdev (the same masked scan); the rank
//                kept in LDS (a byte: < 256), the tile's sent frames and units
//                per netdev in s_tc / s_tu
//   2. once      lane q < nrings turns column q of s_tc into the sent frames of
//                the earlier tiles; rings[q] = {start, count, 0, units} stored
//                whole -- the workgroup owns the batch, so no atomics
//   3. per tile  entry = start + earlier tiles' + rank; the entry stored by the
//                frame's own lane as fwd_desc_store_body stores it
// Phase 3 walks the tiles backwards: the last tile's record, offset and rank
// are still in registers, so a one-tile batch reads nothing twice.  An earlier
// tile's record is re-read from plan[] by the lane that stored it, its rank from
// the byte the same lane wrote.  Every loop's bound (the tiles, <= 32; nrings,
// <= 16; the table sizes) is known at entry, every barrier sits outside lane-
// dependent control flow, and no workgroup waits on another.
#define FWD_ONE_TILES (MOSRX_FWD_ONE_MAX / MOSRX_FWD_TILE)
static_assert(MOSRX_FWD_ONE_MAX % MOSRX_FWD_TILE == 0 && FWD_ONE_TILES == 32u, "one workgroup walks at most 32 tiles");

// Phase 1's share of tile k once its lanes hold their records: netdev, units and
// rank of this lane's frame (the rank also into its byte of s_rank), the tile's
// totals per netdev into row k.  Ends in a barrier: the next tile's scan
// rewrites s_wu / s_wc.
__device__ __forceinline__ void fwd_one_tile_totals(u32x2 pl, uint32_t k, uint32_t nrings, uint32_t (*s_wu)[FWD_NQ],
                                                    uint32_t (*s_wc)[FWD_NQ], uint32_t (*s_tu)[FWD_NQ],
                                                    uint32_t (*s_tc)[FWD_NQ], uint8_t *s_rank, uint32_t &q,
                                                    uint32_t &units, uint32_t &rank)
{
	const uint32_t t = threadIdx.x;
	uint32_t excl;
	units = fwd_ring_units(pl, nrings, q);
	fwd_ring_tile_scan(q, units, nrings, s_wu, s_wc, excl, rank);
	s_rank[k * MOSRX_FWD_TILE + t] = (uint8_t)rank;
	if (t < nrings) {
		uint32_t tu = 0, tc = 0;
#pragma unroll
		for (uint32_t w = 0; w < FWD_WAVES; w++) {
			tu += s_wu[w][t];
			tc += s_wc[w][t];
		}
		s_tu[k][t] = tu;
		s_tc[k][t] = tc;
	}
	__syncthreads();
}

template <uint32_t RB, bool PLAN>
__global__ __launch_bounds__(MOSRX_FWD_THREADS) void mosrx_fwd_one_kernel(mosrx_oparams op)
{
	__shared__ uint32_t s_rm[MOSRX_FWD_MAX_ROUTES], s_rv[MOSRX_FWD_MAX_ROUTES];
	__shared__ int32_t s_rp[MOSRX_FWD_MAX_ROUTES], s_rn[MOSRX_FWD_MAX_ROUTES];
	__shared__ uint32_t s_am[MOSRX_FWD_MAX_ARP], s_av[MOSRX_FWD_MAX_ARP];
	__shared__ int32_t s_ap[MOSRX_FWD_MAX_ARP];
	__shared__ uint32_t s_wu[FWD_WAVES][FWD_NQ], s_wc[FWD_WAVES][FWD_NQ];
	__shared__ uint32_t s_tu[FWD_ONE_TILES][FWD_NQ], s_tc[FWD_ONE_TILES][FWD_NQ];
	__shared__ uint32_t s_tot[FWD_NQ], s_start[FWD_NQ];
	__shared__ uint8_t s_rank[MOSRX_FWD_ONE_MAX];
	if (blockIdx.x >= op.nb)
		return;
	const mosrx_ddesc d = op.ddesc ? op.ddesc[blockIdx.x] : op.oned;
	const uint32_t nrings = min(op.nrings, FWD_NQ);
	const uint32_t t = threadIdx.x;
	const uint32_t tiles = min((d.n + MOSRX_FWD_TILE - 1u) / MOSRX_FWD_TILE, FWD_ONE_TILES);
	mosrx_dparams p = {};   // as the store launch's body takes the batch
	p.frames = d.frames;
	p.off = d.off;
	p.tab = op.tab;
	p.plan = d.plan;
	p.frames_bytes = d.frames_bytes;
	p.n = d.n;
	p.tx_src = d.tx_src;
	p.tx_len = d.tx_len;
	p.tx_mac = d.tx_mac;
	mosrx_fparams fp = {};  // as the plan launch's body takes it
	if constexpr (PLAN) {
		const mosrx_fdesc f = op.fdesc ? op.fdesc[blockIdx.x] : op.onef;
		fp.frames = d.frames;
		fp.off = d.off;
		fp.len = f.len;
		fp.rec = f.rec;
		fp.tab = op.tab;
		fp.plan = f.plan;
		fp.frames_bytes = d.frames_bytes;
		fp.n = d.n;
		fp.in_ifidx = (int32_t)f.in_ifidx;
		fp.forward = op.forward;
		fp.num_msp = op.num_msp;
		fp.listener = op.listener;
	}
	u32x2 pl = {0u, 0u};
	uint32_t fo = 0, q = 0, units = 0, rank = 0;
	if constexpr (PLAN) {
		const mosrx_fparams &p = fp;
#define FWD_PLAN 1
#include "mosrx_fwd_plan_body.inc"
		for (uint32_t k = 0; k < tiles; k++) {
			const uint32_t i = k * MOSRX_FWD_TILE + t;
			pl.x = pl.y = 0u;
			fo = 0;
			if (i < p.n) {
#define FWD_PLAN 2
#include "mosrx_fwd_plan_body.inc"
				*reinterpret_cast<u32x2 *>(p.plan + i) = v;
				pl = v;
				fo = o;
			}
			fwd_one_tile_totals(pl, k, nrings, s_wu, s_wc, s_tu, s_tc, s_rank, q, units, rank);
		}
	} else {
		for (uint32_t k = 0; k < tiles; k++) {
			const uint32_t i = k * MOSRX_FWD_TILE + t;
			pl.x = pl.y = 0u;
			fo = 0;
			if (i < p.n) {
				pl = *reinterpret_cast<const u32x2 *>(p.plan + i);
				fo = p.off[i];
			}
			fwd_one_tile_totals(pl, k, nrings, s_wu, s_wc, s_tu, s_tc, s_rank, q, units, rank);
		}
	}
	// 2. lane q: its column's exclusive prefix over the tiles, its ring's row
	uint32_t cnt = 0, un = 0;
	if (t < nrings) {
		for (uint32_t k = 0; k < tiles; k++) {
			const uint32_t c = s_tc[k][t];
			s_tc[k][t] = cnt;
			cnt += c;
			un += s_tu[k][t];
		}
		s_tot[t] = cnt;
	}
	__syncthreads();
	if (t < nrings) {
		uint32_t start = 0;
		for (uint32_t g = 0; g < nrings; g++)
			start += g < t ? s_tot[g] : 0u;
		s_start[t] = start;
		u32x4 row = {start, cnt, 0u, un};
		*reinterpret_cast<u32x4 *>(d.rings + t) = row;
	}
	__syncthreads();
	// 3. the entries, last tile first
	for (uint32_t k = tiles; k-- > 0u;) {
		const uint32_t i = k * MOSRX_FWD_TILE + t;
		if (k + 1u != tiles) {
			pl.x = pl.y = 0u;
			fo = 0;
			if (i < p.n) {
				pl = *reinterpret_cast<const u32x2 *>(p.plan + i);
				fo = p.off[i];
			}
			units = fwd_ring_units(pl, nrings, q);
			rank = s_rank[i];
		}
		const bool sent = units != 0u;   // (then q < nrings and i < n)
		const uint32_t qq = q & (FWD_NQ - 1u);
		const uint32_t j = s_start[qq] + s_tc[k][qq] + rank;
		if (sent && j < p.n) {
			const uint32_t o = fo;
#include "mosrx_fwd_desc_entry.inc"
		}
	}
}

static int fwd_common_ok(const mosrx_fparams *fp)
{
	return fp && fp->tab && fp->plan && !((uintptr_t)fp->plan & 7) &&
	       (fp->n == 0 || (fp->frames && fp->off && fp->len && !((uintptr_t)fp->off & 3) && !((uintptr_t)fp->len & 1)));
}

extern "C" int mosrx_launch_fwd_plan(const mosrx_fparams *fp, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!fwd_common_ok(fp) || (fp->rec_bytes != 8u && fp->rec_bytes != 16u) || fp->in_ifidx < 0 ||
	    fp->in_ifidx >= MOSRX_FWD_MAX_NETDEVS)
		return -EINVAL;
	if (fp->n == 0)
		return 0;
	if (!fp->rec || ((uintptr_t)fp->rec & (fp->rec_bytes - 1u)))
		return -EINVAL;
	const dim3 grid((fp->n + MOSRX_FWD_THREADS - 1u) / MOSRX_FWD_THREADS), block(MOSRX_FWD_THREADS);
	if (fp->rec_bytes == 8u)
		hipLaunchKernelGGL(mosrx_fwd_plan_kernel<8u>, grid, block, 0, s, *fp);
	else
		hipLaunchKernelGGL(mosrx_fwd_plan_kernel<16u>, grid, block, 0, s, *fp);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_fwd_build(const mosrx_fparams *fp, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!fwd_common_ok(fp) || !fp->tx || ((uintptr_t)fp->tx & 15) || !fp->tx_off || ((uintptr_t)fp->tx_off & 3) ||
	    !fp->tx_len || ((uintptr_t)fp->tx_len & 1) || !fp->tx_nif || !fp->tx_src || ((uintptr_t)fp->tx_src & 3) ||
	    !fp->tx_count || ((uintptr_t)fp->tx_count & 3) || !fp->scratch || ((uintptr_t)fp->scratch & 15) ||
	    fp->tiles != (fp->n + MOSRX_FWD_TILE - 1u) / MOSRX_FWD_TILE)
		return -EINVAL;
	if (fp->tiles)
		hipLaunchKernelGGL(mosrx_fwd_totals_kernel, dim3(fp->tiles), dim3(MOSRX_FWD_THREADS), 0, s, *fp);
	hipLaunchKernelGGL(mosrx_fwd_scan_kernel, dim3(1), dim3(FWD_SCAN_THREADS), 0, s, *fp);
	if (fp->tiles)
		hipLaunchKernelGGL(mosrx_fwd_copy_kernel, dim3(fp->tiles), dim3(MOSRX_FWD_THREADS), 0, s, *fp);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_fwd_rings(const mosrx_rparams *rp, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!rp || !rp->tab || !rp->plan || ((uintptr_t)rp->plan & 7) ||
	    (rp->n && (!rp->frames || !rp->off || ((uintptr_t)rp->off & 3))) || !rp->tx || ((uintptr_t)rp->tx & 15) ||
	    !rp->tx_off || ((uintptr_t)rp->tx_off & 3) || !rp->tx_len || ((uintptr_t)rp->tx_len & 1) || !rp->tx_src ||
	    ((uintptr_t)rp->tx_src & 3) || !rp->rings || ((uintptr_t)rp->rings & 15) || !rp->scratch ||
	    ((uintptr_t)rp->scratch & 15) || rp->nrings < 1u || rp->nrings > FWD_NQ ||
	    (uint64_t)rp->nrings * rp->cap_units > (1ull << 28) ||
	    rp->tiles != (rp->n + MOSRX_FWD_TILE - 1u) / MOSRX_FWD_TILE)
		return -EINVAL;
	if (rp->tiles)
		hipLaunchKernelGGL(mosrx_fwd_ring_totals_kernel, dim3(rp->tiles), dim3(MOSRX_FWD_THREADS), 0, s, *rp);
	hipLaunchKernelGGL(mosrx_fwd_ring_scan_kernel, dim3(1), dim3(FWD_SCAN_THREADS), 0, s, *rp);
	if (rp->tiles)
		hipLaunchKernelGGL(mosrx_fwd_ring_copy_kernel, dim3(rp->tiles), dim3(MOSRX_FWD_THREADS), 0, s, *rp);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// What every queue launch asks of fq, and what a ring build asks on top (host code only).
static int fwd_queue_ok(const mosrx_fqparams *fq)
{
	return fq && fq->desc && fq->tab && fq->nb != 0 && (fq->rec_bytes == 8u || fq->rec_bytes == 16u);
}

static int fwd_queue_build_ok(const mosrx_fqparams *fq)
{
	return fq->scratch && !((uintptr_t)fq->scratch & 15) && fq->nrings >= 1u && fq->nrings <= FWD_NQ;
}

static int fwd_desc_queue_ok(const mosrx_fqparams *fq, const mosrx_dqparams *dq)
{
	return fwd_queue_ok(fq) && fwd_queue_build_ok(fq) && dq && dq->desc && dq->tab == fq->tab &&
	       dq->scratch == fq->scratch && dq->nb == fq->nb && dq->total_tiles == fq->total_tiles &&
	       dq->nrings == fq->nrings;
}

static void fwd_queue_plan_launch(const mosrx_fqparams *fq, hipStream_t s)
{
	const dim3 grid(fq->total_tiles), block(MOSRX_FWD_THREADS);
	if (!fq->total_tiles)
		return;
	if (fq->rec_bytes == 8u)
		hipLaunchKernelGGL(mosrx_fwd_plan_queue_kernel<8u>, grid, block, 0, s, *fq);
	else
		hipLaunchKernelGGL(mosrx_fwd_plan_queue_kernel<16u>, grid, block, 0, s, *fq);
}

// totals, scan (one workgroup per batch), then the byte-ring copy (dq NULL) or the descriptor store
static void fwd_queue_build_launches(const mosrx_fqparams *fq, const mosrx_dqparams *dq, hipStream_t s)
{
	const dim3 grid(fq->total_tiles), block(MOSRX_FWD_THREADS);
	if (fq->total_tiles)
		hipLaunchKernelGGL(mosrx_fwd_ring_totals_queue_kernel, grid, block, 0, s, *fq);
	hipLaunchKernelGGL(mosrx_fwd_ring_scan_queue_kernel, dim3(fq->nb), dim3(FWD_SCAN_THREADS), 0, s, *fq);
	if (!fq->total_tiles)
		return;
	if (dq)
		hipLaunchKernelGGL(mosrx_fwd_desc_store_queue_kernel, grid, block, 0, s, *dq);
	else
		hipLaunchKernelGGL(mosrx_fwd_ring_copy_queue_kernel, grid, block, 0, s, *fq);
}

extern "C" int mosrx_launch_fwd_queue(const mosrx_fqparams *fq, int with_build, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!fwd_queue_ok(fq))
		return -EINVAL;
	if (with_build && (!fwd_queue_build_ok(fq) || (uint64_t)fq->nrings * fq->cap_units > (1ull << 28)))
		return -EINVAL;
	fwd_queue_plan_launch(fq, s);
	if (with_build)
		fwd_queue_build_launches(fq, NULL, s);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_fwd_queue_build(const mosrx_fqparams *fq, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!fwd_queue_ok(fq) || !fwd_queue_build_ok(fq) || (uint64_t)fq->nrings * fq->cap_units > (1ull << 28))
		return -EINVAL;
	fwd_queue_build_launches(fq, NULL, s);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

static int fwd_desc_ok(const mosrx_dparams *dp)
{
	return dp && dp->tab && dp->plan && !((uintptr_t)dp->plan & 7) &&
	       (dp->n == 0 || (dp->frames && dp->off && !((uintptr_t)dp->off & 3))) && dp->tx_src &&
	       !((uintptr_t)dp->tx_src & 3) && dp->tx_len && !((uintptr_t)dp->tx_len & 1) && dp->tx_mac &&
	       !((uintptr_t)dp->tx_mac & 3) && dp->rings && !((uintptr_t)dp->rings & 15) && dp->scratch &&
	       !((uintptr_t)dp->scratch & 15) && dp->nrings >= 1u && dp->nrings <= FWD_NQ &&
	       dp->tiles == (dp->n + MOSRX_FWD_TILE - 1u) / MOSRX_FWD_TILE;
}

extern "C" int mosrx_launch_fwd_desc(const mosrx_dparams *dp, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!fwd_desc_ok(dp))
		return -EINVAL;
	// the ring form's totals and scan read the plan, the scratch rows and the rings only
	mosrx_rparams rp = {};
	rp.plan = dp->plan;
	rp.n = dp->n;
	rp.nrings = dp->nrings;
	rp.tiles = dp->tiles;
	rp.rings = dp->rings;
	rp.scratch = dp->scratch;
	if (dp->tiles)
		hipLaunchKernelGGL(mosrx_fwd_ring_totals_kernel, dim3(dp->tiles), dim3(MOSRX_FWD_THREADS), 0, s, rp);
	hipLaunchKernelGGL(mosrx_fwd_ring_scan_kernel, dim3(1), dim3(FWD_SCAN_THREADS), 0, s, rp);
	if (dp->tiles)
		hipLaunchKernelGGL(mosrx_fwd_desc_store_kernel, dim3(dp->tiles), dim3(MOSRX_FWD_THREADS), 0, s, *dp);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_fwd_desc_queue(const mosrx_fqparams *fq, const mosrx_dqparams *dq, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!fwd_desc_queue_ok(fq, dq))
		return -EINVAL;
	fwd_queue_plan_launch(fq, s);
	fwd_queue_build_launches(fq, dq, s);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_fwd_desc_queue_build(const mosrx_fqparams *fq, const mosrx_dqparams *dq, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!fwd_desc_queue_ok(fq, dq))
		return -EINVAL;
	fwd_queue_build_launches(fq, dq, s);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_fwd_one(const mosrx_oparams *op, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!op || !op->tab || op->nb == 0 || (op->rec_bytes != 0u && op->rec_bytes != 8u && op->rec_bytes != 16u) ||
	    op->nrings < 1u || op->nrings > FWD_NQ || (op->ddesc && op->rec_bytes && !op->fdesc))
		return -EINVAL;
	if (!op->ddesc) {
		const mosrx_ddesc *d = &op->oned;
		const mosrx_fdesc *f = &op->onef;
		if (op->nb != 1u || d->n > MOSRX_FWD_ONE_MAX || !d->rings || ((uintptr_t)d->rings & 15) ||
		    (d->n && (!d->frames || !d->off || ((uintptr_t)d->off & 3) || !d->plan || ((uintptr_t)d->plan & 7) ||
		              !d->tx_src || ((uintptr_t)d->tx_src & 3) || !d->tx_len || ((uintptr_t)d->tx_len & 1) ||
		              !d->tx_mac || ((uintptr_t)d->tx_mac & 3))))
			return -EINVAL;
		if (op->rec_bytes && (f->in_ifidx >= MOSRX_FWD_MAX_NETDEVS ||
		                      (d->n && (f->plan != d->plan || !f->len || ((uintptr_t)f->len & 1) || !f->rec ||
		                                ((uintptr_t)f->rec & (op->rec_bytes - 1u))))))
			return -EINVAL;
	}
	const dim3 grid(op->nb), block(MOSRX_FWD_THREADS);
	if (op->rec_bytes == 0u)
		hipLaunchKernelGGL((mosrx_fwd_one_kernel<8u, false>), grid, block, 0, s, *op);
	else if (op->rec_bytes == 8u)
		hipLaunchKernelGGL((mosrx_fwd_one_kernel<8u, true>), grid, block, 0, s, *op);
	else
		hipLaunchKernelGGL((mosrx_fwd_one_kernel<16u, true>), grid, block, 0, s, *op);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
