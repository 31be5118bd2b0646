// mosrx_nat.hip — samples/nat's per-frame work on the frames a forward = 1 stack
// passes on, over a classified batch, in a code object of its own (the plan,
// build, firewall and classify kernels are pinned against their earlier
// disassembly and do not change with it).
//
//   plan-nat  one launch in place of the plan launch; one lane per frame, 256
//             frames per workgroup.
//     1. the route / ARP tables to LDS, as the plan launch copies them
//        (mosrx_fwd_plan_body.inc part 1); one barrier.
//     2. eligibility from the record's last dword (TCP_OK under num_msp != 0 and
//        no listener) and the plan's ip_ok; doff < 5 or a segment under 20 bytes
//        is for the host.  An eligible lane loads its key -- saddr, daddr, the
//        ports' dword at 14 + 4 * ihl -- and the check word, each as two aligned
//        dwords through the batch's buffer resource realigned with v_alignbyte
//        (zero past the end).
//     3. the lookup: open addressing in global memory (64510 bindings are 8 MiB
//        of slots: not LDS), 16 bytes a probe and 8 more on the hit; at most
//        `probe` steps, the host's recorded longest run, and a wave leaves when
//        a ballot shows no lane still looking.
//     4. a translated lane recomputes ip_fast_csum over its 5 .. 15 header dwords
//        with the new address in place, and takes the TCP check from the old
//        check word alone (mosrx_nat.h).
//     5. the plan record by the plan launch's own text (part 2), its daddr the
//        translated one for DNAT; MISS / HOST frames get their own kinds.  One
//        8-byte and one 16-byte store per frame.
//   patch     one lane per ring entry behind the byte-ring build: an entry of a
//             ring's written run whose frame was translated gets its four fields
//             stored into the built frame (2- and 4-byte stores: ring frames sit
//             at 16 k + 2).
//   update    one lane per changed slot of the table (mosrx_nat_update): the
//             host did the table's arithmetic and made the slots distinct; a
//             lane stores one 32-byte image.  No loop, no LDS, no atomics.
// A slot whose kind is MOSRX_NAT_TOMB held a key that was deleted: the lookup
// steps over it, where a free slot ends the run.
// No workgroup waits on another; every loop's bound (the table sizes, probe,
// ihl <= 15, nrings <= 16, the queue's batch search) is known at its entry;
// every frame read goes through the buffer resource; every per-frame store sits
// under i < n, every patch store under e < n inside a ring's written run.  All
// stores are vector stores.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "mosrx_device.h"
#include "mosrx_nat.h"

static_assert(MOSRX_NAT_TILE == MOSRX_NAT_THREADS && MOSRX_NAT_TILE == 256u && MOSRX_FWD_THREADS == 256u,
              "one lane per frame; the forwarding tile");
static_assert(sizeof(mosrx_fwd) == 8 && sizeof(mosrx_nat_xlat) == 16 && sizeof(mosrx_nat_slot) == 32 &&
              sizeof(mosrx_fwd_ring) == 16, "8-byte plan records, 16-byte xlat records, 32-byte slots, 16-byte ring rows");
static_assert(offsetof(mosrx_nat_slot, port) == 12 && offsetof(mosrx_nat_slot, kind) == 14 &&
              offsetof(mosrx_nat_slot, addr) == 16 && offsetof(mosrx_nat_slot, bind) == 20, "slot halves");
static_assert(offsetof(mosrx_nat_xlat, port) == 4 && offsetof(mosrx_nat_xlat, ip_check) == 6 &&
              offsetof(mosrx_nat_xlat, tcp_check) == 8 && offsetof(mosrx_nat_xlat, kind) == 10 &&
              offsetof(mosrx_nat_xlat, ihl) == 11 && offsetof(mosrx_nat_xlat, bind) == 12, "xlat dwords");
static_assert(sizeof(mosrx_nat_touch) == 48 && offsetof(mosrx_nat_touch, image) == 16, "a touch entry: three 16-byte loads");

// bytes a .. a+3 of the batch buffer, any alignment (zero past its end); the name
// mosrx_fwd_plan_body.inc calls
__device__ __forceinline__ uint32_t fwd_ld32(__amdgpu_buffer_rsrc_t r, uint32_t a)
{
	const uint32_t a4 = a & ~3u;
	const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(r, a4, 0, 0);
	const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(r, a4 + 4u, 0, 0);
	return __builtin_amdgcn_alignbyte(hi, lo, a & 3u);
}

// what the plan routes: a DNAT frame's translated daddr, else the frame's own
#define FWD_PLAN_DADDR (x_kind == MOSRX_NAT_DNAT ? x_addr : fwd_ld32(rs, o + 30u))

// ---- plan-nat ----------------------------------------------------------------
// Workgroup `blk` of the batch in p: frames blk * 256 ..  RB: the record size.
template <uint32_t RB>
__device__ __forceinline__ void nat_plan_body(const mosrx_fparams p, const mosrx_nat_slot *slots, uint32_t mask,
                                              uint32_t probe, mosrx_nat_xlat *xlat, uint32_t blk)
{
	__shared__ uint32_t s_rm[MOSRX_FWD_MAX_ROUTES], s_rv[MOSRX_FWD_MAX_ROUTES];
	__shared__ int32_t s_rp[MOSRX_FWD_MAX_ROUTES], s_rn[MOSRX_FWD_MAX_ROUTES];
	__shared__ uint32_t s_am[MOSRX_FWD_MAX_ARP], s_av[MOSRX_FWD_MAX_ARP];
	__shared__ int32_t s_ap[MOSRX_FWD_MAX_ARP];
	const uint32_t t = threadIdx.x, i = blk * MOSRX_NAT_THREADS + t;
#define FWD_PLAN 1
#include "mosrx_fwd_plan_body.inc"

	// 2. eligibility, the key and the old check word
	uint32_t x_kind = MOSRX_NAT_NONE, x_ihl = 0, x_addr = 0, x_port = 0, x_bind = 0;
	uint32_t k_o = 0, k_sa = 0, k_da = 0, k_pt = 0, k_chk = 0;
	bool looking = false;
	if (i < p.n) {
		const uint32_t k_reason = *reinterpret_cast<const uint32_t *>(p.rec + (uint64_t)i * RB + (RB - 4u)) & 0xFFu;
		// the TCP arm of mosrx_mos_forwards (csrc/rx_loop.c) for an accepted segment
		if (k_reason == MOSRX_R_TCP_OK && p.num_msp != 0 && !p.listener) {
			k_o = p.off[i];
			const uint32_t k_cap = eff_caplen(k_o, p.len[i], p.frames_bytes);
			const __amdgpu_buffer_rsrc_t k_rs = frame_rsrc(p.frames, p.frames_bytes);
			const uint32_t w_ihl = fwd_ld32(k_rs, k_o + 14u);   // version / ihl byte, tos, tot_len (network order)
			const uint32_t k_len = ((w_ihl >> 8) & 0xFF00u) | (w_ihl >> 24);
			// the plan's ip_ok: the IPv4 packet lies inside the capture
			if (k_cap >= 34u && k_len >= 20u && 14u + k_len <= k_cap) {
				x_ihl = w_ihl & 0xFu;
				x_bind = MOSRX_NAT_NO_BIND;
				const uint32_t th = k_o + 14u + 4u * x_ihl;
				const uint32_t doff = (fwd_ld32(k_rs, th + 12u) >> 4) & 0xFu;
				if (doff < 5u || k_len < 4u * x_ihl + 20u) {
					x_kind = MOSRX_NAT_HOST;
				} else {
					x_kind = MOSRX_NAT_MISS;
					looking = true;
					k_sa = fwd_ld32(k_rs, k_o + 26u);
					k_da = fwd_ld32(k_rs, k_o + 30u);
					k_pt = fwd_ld32(k_rs, th);                  // source | dest << 16, as the sample's offsets see them
					k_chk = fwd_ld32(k_rs, th + 16u) & 0xFFFFu; // tcph->check as received
				}
			}
		}
	}

	// 3. the lookup
	const uint32_t h = mosrx_nat_hash_key(k_sa, k_da, k_pt);
	for (uint32_t d = 0; d < probe; d++) {
		if (__ballot(looking) == 0ull)
			break;
		if (looking) {
			const mosrx_nat_slot *s = slots + ((h + d) & mask);
			const u32x4 k = *reinterpret_cast<const u32x4 *>(s);
			const uint32_t sk = (k.w >> 16) & 0xFFu;
			if (sk != MOSRX_NAT_SNAT && sk != MOSRX_NAT_DNAT) {
				looking = sk == MOSRX_NAT_TOMB;                 // a free slot ends the run: no binding; a deleted key's is stepped over
			} else if (k.x == k_sa && k.y == k_da && k.z == k_pt) {
				const u32x2 val = *reinterpret_cast<const u32x2 *>(&s->addr);
				x_kind = sk;
				x_port = k.w & 0xFFFFu;
				x_addr = val.x;
				x_bind = val.y;
				looking = false;
			}
		}
	}
	if (i >= p.n)
		return;

	// 4. the checksums of a translated frame
	uint32_t ipc = 0, tcpc = 0;
	if (x_kind == MOSRX_NAT_SNAT || x_kind == MOSRX_NAT_DNAT) {
		const __amdgpu_buffer_rsrc_t k_rs = frame_rsrc(p.frames, p.frames_bytes);
		const uint32_t a = k_o + 14u, a4 = a & ~3u, sh = a & 3u;
		uint32_t prev = __builtin_amdgcn_raw_buffer_load_b32(k_rs, a4, 0, 0);
		uint64_t acc = 0;
		for (uint32_t j = 0; j < x_ihl; j++) {                  // x_ihl <= 15
			const uint32_t next = __builtin_amdgcn_raw_buffer_load_b32(k_rs, a4 + 4u * (j + 1u), 0, 0);
			const uint32_t w = __builtin_amdgcn_alignbyte(next, prev, sh);
			prev = next;
			acc = mosrx_nat_ip_acc(acc, mosrx_nat_ip_word(j, w, x_kind, x_addr));
		}
		ipc = mosrx_nat_ip_fold(acc);
		const bool snat = x_kind == MOSRX_NAT_SNAT;
		tcpc = mosrx_nat_tcp_check(snat ? k_sa : k_da, x_addr, snat ? k_pt & 0xFFFFu : k_pt >> 16, x_port, k_chk);
	}

	// 5. the plan record and the xlat record
	{
#define FWD_PLAN 2
#include "mosrx_fwd_plan_body.inc"
		if (p.forward && (x_kind == MOSRX_NAT_MISS || x_kind == MOSRX_NAT_HOST)) {
			const uint32_t fk = x_kind == MOSRX_NAT_MISS ? (uint32_t)MOSRX_FWD_NAT_MISS : (uint32_t)MOSRX_FWD_NAT_HOST;
			v.x = (0xFFu << 16) | (fk << 24);   // tx_len 0, out_ifidx -1
			v.y = 0xFFFFu;                      // arp_idx none, reserved 0
		}
		*reinterpret_cast<u32x2 *>(p.plan + i) = v;
	}
	u32x4 x;
	x.x = x_addr;
	x.y = x_port | (ipc << 16);
	x.z = tcpc | (x_kind << 16) | (x_ihl << 24);
	x.w = x_bind;
	*reinterpret_cast<u32x4 *>(xlat + i) = x;
}

template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_NAT_THREADS) void mosrx_nat_plan_kernel(mosrx_nparams np)
{
	nat_plan_body<RB>(np.f, np.slots, np.mask, np.probe, np.xlat, blockIdx.x);
}

// The batch of tile `blk` of a queue launch: find k with tile_base[k] <= blk <
// tile_base[k+1], as the forwarding queue kernels do (empty batches share their
// successor's base and are skipped).  The bound is known at entry and the
// search is uniform over the workgroup.
__device__ __forceinline__ uint32_t nat_queue_batch(const mosrx_fdesc *desc, uint32_t nb, uint32_t blk)
{
	uint32_t lo = 0, hi = nb;
	for (int it = 0; it < 32 && hi - lo > 1; it++) {
		const uint32_t mid = (lo + hi) >> 1;
		if (desc[mid].tile_base <= blk)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_NAT_THREADS) void mosrx_nat_plan_queue_kernel(mosrx_nparams np)
{
	if (blockIdx.x >= np.total_tiles)
		return;
	const uint32_t k = nat_queue_batch(np.fdesc, np.nb, blockIdx.x);
	const mosrx_fdesc d = np.fdesc[k];
	mosrx_fparams p = {};
	p.frames = d.frames;
	p.off = d.off;
	p.len = d.len;
	p.rec = d.rec;
	p.tab = np.f.tab;
	p.plan = d.plan;
	p.frames_bytes = d.frames_bytes;
	p.n = d.n;
	p.in_ifidx = (int32_t)d.in_ifidx;
	p.forward = np.f.forward;
	p.num_msp = np.f.num_msp;
	p.listener = np.f.listener;
	nat_plan_body<RB>(p, np.slots, np.mask, np.probe, np.xtab[k], blockIdx.x - d.tile_base);
}

// ---- patch -------------------------------------------------------------------
// Entry e = blk * 256 + lane of one batch's ring build outputs.
__device__ __forceinline__ void nat_patch_body(const mosrx_nat_xlat *xlat, uint8_t *tx, const uint32_t *tx_off,
                                               const uint32_t *tx_src, const mosrx_fwd_ring *rings, uint32_t nrings,
                                               uint32_t n, uint32_t blk)
{
	const uint32_t e = blk * MOSRX_NAT_THREADS + threadIdx.x;
	if (e >= n)
		return;
	// the ring whose written run holds e; entries of dropped frames and entries past the last ring are not frames
	const uint32_t nr = min(nrings, (uint32_t)MOSRX_FWD_MAX_NETDEVS);
	bool live = false;
	for (uint32_t g = 0; g < nr; g++) {
		const u32x4 r = *reinterpret_cast<const u32x4 *>(rings + g);   // start, count, dropped, units
		live = live || e - r.x < r.y;                                    // (unsigned: start <= e < start + count)
	}
	if (!live)
		return;
	const uint32_t i = tx_src[e];
	if (i >= n)
		return;
	const u32x4 x = *reinterpret_cast<const u32x4 *>(xlat + i);
	const uint32_t kind = (x.z >> 16) & 0xFFu, ihl = x.z >> 24 & 0xFu;
	const uint32_t o = tx_off[e];
	if ((kind != MOSRX_NAT_SNAT && kind != MOSRX_NAT_DNAT) || (o & 15u) != 2u)   // (a built frame sits at 16 k + 2)
		return;
	const bool snat = kind == MOSRX_NAT_SNAT;
	uint8_t *f = tx + o;
	const uint32_t th = 14u + 4u * ihl;
	*reinterpret_cast<uint16_t *>(f + 24u) = (uint16_t)(x.y >> 16);
	*reinterpret_cast<uint32_t *>(f + (snat ? 26u : 30u)) = x.x;
	*reinterpret_cast<uint16_t *>(f + th + (snat ? 0u : 2u)) = (uint16_t)x.y;
	*reinterpret_cast<uint16_t *>(f + th + 16u) = (uint16_t)x.z;
}

__global__ __launch_bounds__(MOSRX_NAT_THREADS) void mosrx_nat_patch_kernel(mosrx_npatch pp)
{
	nat_patch_body(pp.xlat, pp.tx, pp.tx_off, pp.tx_src, pp.rings, pp.nrings, pp.n, blockIdx.x);
}

__global__ __launch_bounds__(MOSRX_NAT_THREADS) void mosrx_nat_patch_queue_kernel(mosrx_npatch pp)
{
	if (blockIdx.x >= pp.total_tiles)
		return;
	const uint32_t k = nat_queue_batch(pp.fdesc, pp.nb, blockIdx.x);
	const mosrx_fdesc d = pp.fdesc[k];
	nat_patch_body(pp.xtab[k], d.tx, d.tx_off, d.tx_src, d.rings, pp.nrings, d.n, blockIdx.x - d.tile_base);
}

// ---- update ------------------------------------------------------------------
// Lane i stores the image of touch[i] into its slot: three 16-byte loads (the
// slot index, the image's halves), two 16-byte stores under i < m and slot <= mask.
// The value half goes first and the key half, which holds the kind, behind it;
// the ordering that counts is the stream's (include/mosrx.h mosrx_nat_update).
__global__ __launch_bounds__(MOSRX_NAT_THREADS) void mosrx_nat_update_kernel(mosrx_nat_slot *slots, uint32_t mask,
                                                                            const mosrx_nat_touch *touch, uint32_t m)
{
	const uint32_t i = blockIdx.x * MOSRX_NAT_THREADS + threadIdx.x;
	if (i >= m)
		return;
	const u32x4 *t = reinterpret_cast<const u32x4 *>(touch + i);
	const u32x4 hd = t[0], key = t[1], val = t[2];
	if (hd.x > mask)
		return;
	u32x4 *s = reinterpret_cast<u32x4 *>(slots + hd.x);
	s[1] = val;
	s[0] = key;
}

// ---- launches ----------------------------------------------------------------
extern "C" int mosrx_launch_nat_update(mosrx_nat_slot *slots, uint32_t mask, const mosrx_nat_touch *touch, uint32_t m,
                                       void *stream)
{
	if (!slots || ((uintptr_t)slots & 15) || !touch || ((uintptr_t)touch & 15) || (mask & (mask + 1u)) ||
	    mask + 1u < MOSRX_NAT_MIN_SLOTS)
		return -EINVAL;
	if (m == 0)
		return 0;
	hipLaunchKernelGGL(mosrx_nat_update_kernel, dim3((m + MOSRX_NAT_THREADS - 1u) / MOSRX_NAT_THREADS),
	                   dim3(MOSRX_NAT_THREADS), 0, (hipStream_t)stream, slots, mask, touch, m);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_nat_plan(const mosrx_nparams *np, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!np || !np->f.tab || !np->slots || ((uintptr_t)np->slots & 15) || (np->mask & (np->mask + 1u)) ||
	    np->mask + 1u < MOSRX_NAT_MIN_SLOTS || (np->f.rec_bytes != 8u && np->f.rec_bytes != 16u))
		return -EINVAL;
	if (np->fdesc) {
		if (!np->xtab || np->nb == 0)
			return -EINVAL;
		if (np->total_tiles == 0)
			return 0;
		const dim3 grid(np->total_tiles), block(MOSRX_NAT_THREADS);
		if (np->f.rec_bytes == 8u)
			hipLaunchKernelGGL(mosrx_nat_plan_queue_kernel<8u>, grid, block, 0, s, *np);
		else
			hipLaunchKernelGGL(mosrx_nat_plan_queue_kernel<16u>, grid, block, 0, s, *np);
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	const mosrx_fparams *fp = &np->f;
	if (!fp->plan || ((uintptr_t)fp->plan & 7) || !np->xlat || ((uintptr_t)np->xlat & 15) || fp->in_ifidx < 0 ||
	    fp->in_ifidx >= MOSRX_FWD_MAX_NETDEVS)
		return -EINVAL;
	if (fp->n == 0)
		return 0;
	if (!fp->frames || !fp->off || ((uintptr_t)fp->off & 3) || !fp->len || ((uintptr_t)fp->len & 1) || !fp->rec ||
	    ((uintptr_t)fp->rec & (fp->rec_bytes - 1u)))
		return -EINVAL;
	const dim3 grid((fp->n + MOSRX_NAT_THREADS - 1u) / MOSRX_NAT_THREADS), block(MOSRX_NAT_THREADS);
	if (fp->rec_bytes == 8u)
		hipLaunchKernelGGL(mosrx_nat_plan_kernel<8u>, grid, block, 0, s, *np);
	else
		hipLaunchKernelGGL(mosrx_nat_plan_kernel<16u>, grid, block, 0, s, *np);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mosrx_launch_nat_patch(const mosrx_npatch *pp, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!pp || pp->nrings < 1u || pp->nrings > MOSRX_FWD_MAX_NETDEVS)
		return -EINVAL;
	if (pp->fdesc) {
		if (!pp->xtab || pp->nb == 0)
			return -EINVAL;
		if (pp->total_tiles == 0)
			return 0;
		hipLaunchKernelGGL(mosrx_nat_patch_queue_kernel, dim3(pp->total_tiles), dim3(MOSRX_NAT_THREADS), 0, s, *pp);
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	if (!pp->xlat || ((uintptr_t)pp->xlat & 15) || !pp->tx || ((uintptr_t)pp->tx & 15) || !pp->tx_off ||
	    ((uintptr_t)pp->tx_off & 3) || !pp->tx_src || ((uintptr_t)pp->tx_src & 3) || !pp->rings ||
	    ((uintptr_t)pp->rings & 15))
		return -EINVAL;
	if (pp->n == 0)
		return 0;
	hipLaunchKernelGGL(mosrx_nat_patch_kernel, dim3((pp->n + MOSRX_NAT_THREADS - 1u) / MOSRX_NAT_THREADS),
	                   dim3(MOSRX_NAT_THREADS), 0, s, *pp);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
