// mosrx_acl.hip — samples/simple_firewall's rule on the frames a forward = 1
// stack passes on, over a classified batch: one launch, in a code object of its
// own (the plan, build and classify kernels are pinned against their earlier
// disassembly and do not change with it).
//
//   One lane per frame, 256 frames per workgroup.
//   1. eligibility, from the record's last dword and -- only where that says an
//      accepted TCP frame with SYN and no ACK -- the frame's off / len and its
//      tot_len (the plan's ip_ok).  An eligible lane loads its key: saddr, daddr
//      and the ports' dword at 14 + 4 * ihl, each as two aligned dwords through
//      the batch's buffer resource realigned with v_alignbyte (zero past the end).
//   2. a workgroup without an eligible lane stores 0xFFFF per frame and ends:
//      no table is read (the common case: config #2's trace has no SYN).
//   3. else the rules go to LDS (a b128 + a b64 per rule) and the bins are
//      zeroed; one barrier; each wave with an eligible lane walks rules
//      0 .. n - 1 (every lane reads the same rule per step: a broadcast read),
//      first match wins (FWRLookup, simple_firewall.c:307-330), and leaves the
//      loop when a ballot shows no lane still looking.
//   4. hit[i] stored; under forward, a DROP rule's frame gets the MOSRX_FWD_DROP
//      plan record; one LDS atomic per hit, then one global atomic add per bin
//      that is not zero (a sum: the order does not matter).
// No workgroup waits on another; every loop's bound is known at its entry; every
// per-frame store is under i < n, every counts store under j < the rule count
// <= MOSRX_ACL_MAX_RULES.  All stores are vector stores.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "mosrx_device.h"
#include "mosrx_acl.h"

static_assert(MOSRX_ACL_TILE == MOSRX_ACL_THREADS && MOSRX_ACL_TILE == 256u, "one lane per frame; the forwarding tile");
static_assert(sizeof(mosrx_fwd) == 8, "8-byte plan records");

#define ACL_SYN 0x02u
#define ACL_ACK 0x10u

// bytes a .. a+3 of the batch buffer, any alignment (zero past its end)
__device__ __forceinline__ uint32_t acl_ld32(__amdgpu_buffer_rsrc_t r, uint32_t a)
{
	const uint32_t a4 = a & ~3u;
	const uint32_t lo = __builtin_amdgcn_raw_buffer_load_b32(r, a4, 0, 0);
	const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(r, a4 + 4u, 0, 0);
	return __builtin_amdgcn_alignbyte(hi, lo, a & 3u);
}

// Workgroup `blk` of one batch: frames blk * 256 ..  RB: the record size.
template <uint32_t RB>
__device__ __forceinline__ void acl_body(const mosrx_aparams &p, const uint8_t *frames, const uint32_t *off,
                                         const uint16_t *len, const uint8_t *rec, mosrx_fwd *plan, uint16_t *hit,
                                         uint32_t frames_bytes, uint32_t n, uint32_t blk)
{
	__shared__ u32x4 s_ip[MOSRX_ACL_MAX_RULES];     // src_ip, src_mask, dst_ip, dst_mask
	__shared__ u32x2 s_pt[MOSRX_ACL_MAX_RULES];     // ports, port_mask
	__shared__ uint32_t s_bin[MOSRX_ACL_MAX_RULES];
	const uint32_t t = threadIdx.x, i = blk * MOSRX_ACL_THREADS + t;
	const mosrx_acl_dev *T = p.tab;

	bool elig = false;
	uint32_t sa = 0, da = 0, pt = 0;
	if (i < n) {
		// the record's last dword: reason in byte 0, tcp_flags in byte 2 (16-byte records) or 3 (8-byte)
		const uint32_t w = *reinterpret_cast<const uint32_t *>(rec + (uint64_t)i * RB + (RB - 4u));
		const uint32_t reason = w & 0xFFu, flags = (RB == 16u ? w >> 16 : w >> 24) & 0xFFu;
		// the TCP arm of mosrx_mos_forwards (csrc/rx_loop.c), then CatchInitSYN
		const bool tcp = (reason == MOSRX_R_TCP_OK || reason == MOSRX_R_TCP_LEN_OK) && p.num_msp != 0 && !p.listener;
		if (tcp && (flags & (ACL_SYN | ACL_ACK)) == ACL_SYN) {
			const uint32_t o = off[i];
			const uint32_t cap = eff_caplen(o, len[i], frames_bytes);
			const __amdgpu_buffer_rsrc_t rs = frame_rsrc(frames, frames_bytes);
			const uint32_t w_ihl = acl_ld32(rs, o + 14u);     // version / ihl byte, tos, tot_len (network order)
			const uint32_t ip_len = ((w_ihl >> 8) & 0xFF00u) | (w_ihl >> 24);
			// the plan's ip_ok: the IPv4 packet lies inside the capture
			elig = cap >= 34u && ip_len >= 20u && 14u + ip_len <= cap;
			if (elig) {
				sa = acl_ld32(rs, o + 26u);
				da = acl_ld32(rs, o + 30u);
				pt = acl_ld32(rs, o + 14u + 4u * (w_ihl & 0xFu));   // source | dest << 16, as the sample loads them
			}
		}
	}
	if (!__syncthreads_or(elig)) {
		if (i < n)
			hit[i] = (uint16_t)MOSRX_ACL_NOT_LOOKED_UP;
		return;
	}

	const uint32_t nr = min(T->n, (uint32_t)MOSRX_ACL_MAX_RULES);
	for (uint32_t j = t; j < nr; j += MOSRX_ACL_THREADS) {
		u32x4 a;
		u32x2 b;
		a.x = T->src_ip[j];
		a.y = T->src_mask[j];
		a.z = T->dst_ip[j];
		a.w = T->dst_mask[j];
		b.x = T->ports[j];
		b.y = T->port_mask[j];
		s_ip[j] = a;
		s_pt[j] = b;
		s_bin[j] = 0u;
	}
	__syncthreads();

	uint32_t h = elig ? MOSRX_ACL_NO_MATCH : MOSRX_ACL_NOT_LOOKED_UP;
	bool looking = elig;
	if (__ballot(looking) != 0ull) {
		for (uint32_t j = 0; j < nr; j++) {
			const u32x4 a = s_ip[j];
			const u32x2 b = s_pt[j];
			const bool m = looking && (sa & a.y) == a.x && (da & a.w) == a.z && (pt & b.y) == b.x;
			if (m) {
				h = j;
				looking = false;
			}
			if (__ballot(looking) == 0ull)
				break;
		}
	}
	const bool matched = h < nr;
	if (i < n) {
		hit[i] = (uint16_t)h;
		if (plan && p.forward && matched && T->action[h] == MOSRX_ACL_DROP) {
			u32x2 v;
			v.x = (0xFFu << 16) | ((uint32_t)MOSRX_FWD_DROP << 24);   // tx_len 0, out_ifidx -1
			v.y = 0xFFFFu;                                            // arp_idx none, reserved 0
			*reinterpret_cast<u32x2 *>(plan + i) = v;
		}
	}
	if (p.counts) {
		if (matched)
			atomicAdd(&s_bin[h], 1u);
		__syncthreads();
		for (uint32_t j = t; j < nr; j += MOSRX_ACL_THREADS) {
			const uint32_t c = s_bin[j];
			if (c)
				atomicAdd(p.counts + j, c);
		}
	}
}

template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_ACL_THREADS) void mosrx_acl_kernel(mosrx_aparams p)
{
	acl_body<RB>(p, p.frames, p.off, p.len, p.rec, p.plan, p.hit, p.frames_bytes, p.n, blockIdx.x);
}

// The batch-queue form: find k with tile_base[k] <= blk < tile_base[k+1], as the
// forwarding queue kernels do (empty batches share their successor's base and
// are skipped).  The bound is known at entry and the search is uniform over the
// workgroup.
template <uint32_t RB>
__global__ __launch_bounds__(MOSRX_ACL_THREADS) void mosrx_acl_queue_kernel(mosrx_aparams p)
{
	if (blockIdx.x >= p.total_tiles)
		return;
	uint32_t lo = 0, hi = p.nb;
	for (int it = 0; it < 32 && hi - lo > 1; it++) {
		const uint32_t mid = (lo + hi) >> 1;
		if (p.adesc[mid].tile_base <= blockIdx.x)
			lo = mid;
		else
			hi = mid;
	}
	const mosrx_adesc d = p.adesc[lo];
	mosrx_fwd *plan = p.fdesc ? p.fdesc[lo].plan : NULL;
	acl_body<RB>(p, d.frames, d.off, d.len, d.rec, plan, d.hit, d.frames_bytes, d.n, blockIdx.x - d.tile_base);
}

extern "C" int mosrx_launch_acl(const mosrx_aparams *ap, void *stream)
{
	const hipStream_t s = (hipStream_t)stream;
	if (!ap || !ap->tab || (ap->rec_bytes != 8u && ap->rec_bytes != 16u) || ((uintptr_t)ap->counts & 3))
		return -EINVAL;
	if (ap->adesc) {
		if (ap->nb == 0)
			return -EINVAL;
		if (ap->total_tiles == 0)
			return 0;
		const dim3 grid(ap->total_tiles), block(MOSRX_ACL_THREADS);
		if (ap->rec_bytes == 8u)
			hipLaunchKernelGGL(mosrx_acl_queue_kernel<8u>, grid, block, 0, s, *ap);
		else
			hipLaunchKernelGGL(mosrx_acl_queue_kernel<16u>, grid, block, 0, s, *ap);
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	if (!ap->hit || ((uintptr_t)ap->hit & 1) || ((uintptr_t)ap->plan & 7))
		return -EINVAL;
	if (ap->n == 0)
		return 0;
	if (!ap->frames || !ap->off || ((uintptr_t)ap->off & 3) || !ap->len || ((uintptr_t)ap->len & 1) || !ap->rec ||
	    ((uintptr_t)ap->rec & (ap->rec_bytes - 1u)))
		return -EINVAL;
	const dim3 grid((ap->n + MOSRX_ACL_THREADS - 1u) / MOSRX_ACL_THREADS), block(MOSRX_ACL_THREADS);
	if (ap->rec_bytes == 8u)
		hipLaunchKernelGGL(mosrx_acl_kernel<8u>, grid, block, 0, s, *ap);
	else
		hipLaunchKernelGGL(mosrx_acl_kernel<16u>, grid, block, 0, s, *ap);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
