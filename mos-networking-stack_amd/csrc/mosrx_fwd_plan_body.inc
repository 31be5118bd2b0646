// mosrx_fwd_plan_body.inc — the plan of one frame, included into the plan kernels'
// body (fwd_plan_body) and into the one-launch kernel (mosrx_fwd.hip).  Text, not
// functions, for the reason mosrx_fwd_rings_body.inc gives: the plan kernels are
// pinned against their earlier disassembly.  In scope at the include:
//   p         a mosrx_fparams: the batch, its records, the tables and the rule's parameters
//   s_rm ..   the seven LDS table arrays
//   FWD_PLAN  1 tables: t = threadIdx.x in scope; declares T, nr, na, nicout, walk,
//               copies the walked tables into LDS and ends in a barrier
//             2 record: i < p.n and part 1's names in scope; declares o (the frame's
//               offset) and v, the two dwords of plan[i] (not stored here)
//   FWD_PLAN_DADDR  the address part 2 routes and ARP-resolves; unless the
//               including file defines it (the NAT plan: the translated daddr), the
//               frame's own (rs and o are in scope where it is evaluated)
#ifndef FWD_PLAN_DADDR
#define FWD_PLAN_DADDR fwd_ld32(rs, o + 30u)
#endif
#if FWD_PLAN == 1
	const mosrx_fwd_dev *T = p.tab;
	const uint32_t nr = min(T->num_routes, (uint32_t)MOSRX_FWD_MAX_ROUTES);
	const uint32_t na = min(T->num_arp, (uint32_t)MOSRX_FWD_MAX_ARP);
	// nic_forward_table[in_ifidx], -1 without a table: uniform over the batch
	const int32_t nicout = T->has_nic_fwd ? (int32_t)T->nic_fwd[p.in_ifidx & (MOSRX_FWD_MAX_NETDEVS - 1)] : -1;
	const bool walk = nicout == -1;   // else ForwardIPPacket's fast path: no table is read
	if (walk) {
		for (uint32_t j = t; j < nr; j += MOSRX_FWD_THREADS) {
			s_rm[j] = T->r_mask[j];
			s_rv[j] = T->r_masked[j];
			s_rp[j] = T->r_prefix[j];
			s_rn[j] = T->r_nif[j];
		}
		for (uint32_t j = t; j < na; j += MOSRX_FWD_THREADS) {
			s_am[j] = T->a_mask[j];
			s_av[j] = T->a_masked[j];
			s_ap[j] = T->a_prefix[j];
		}
	}
	__syncthreads();
#elif FWD_PLAN == 2
	const uint32_t reason = *reinterpret_cast<const uint32_t *>(p.rec + (uint64_t)i * RB + (RB - 4u)) & 0xFFu;
	const uint32_t o = p.off[i];
	const uint32_t cap = eff_caplen(o, p.len[i], p.frames_bytes);
	const __amdgpu_buffer_rsrc_t rs = frame_rsrc(p.frames, p.frames_bytes);
	const uint32_t w_len = fwd_ld32(rs, o + 16u);     // iph->tot_len (network order) in the low half
	const uint32_t daddr = FWD_PLAN_DADDR;            // iph->daddr as mOS loads it
	const uint32_t ip_len = ((w_len & 0xFFu) << 8) | ((w_len >> 8) & 0xFFu);
	// mosrx_mos_forwards (csrc/rx_loop.c)
	const uint32_t bit = 1u << reason;
	const uint32_t m_msp = (1u << MOSRX_R_NON_IPV4) | (1u << MOSRX_R_ARP) | (1u << MOSRX_R_NOT_TCP) |
	                       (1u << MOSRX_R_TCP_BADCSUM);
	const uint32_t m_tcp = (1u << MOSRX_R_TCP_OK) | (1u << MOSRX_R_TCP_LEN_OK);
	bool fwd = false;
	if (reason < MOSRX_R_COUNT)
		fwd = (bit & m_msp) ? p.num_msp != 0
		    : (bit & m_tcp) ? (p.num_msp != 0 && !p.listener)
		    : reason == MOSRX_R_NOVERIFY_PASS;
	fwd = fwd && p.forward;
	const bool eth = reason == MOSRX_R_NON_IPV4 || reason == MOSRX_R_ARP;
	// an IPv4 frame whose packet does not lie inside the capture is TRUNCATED or
	// IP_SHORT to the classify kernels: never forwarded, whatever the record says
	const bool ip_ok = cap >= 34u && ip_len >= 20u && 14u + ip_len <= cap;

	// GetOutputInterface: from prefix -1, strictly greater wins
	int32_t best = -1, nif = -1;
	// GetDestinationHWaddr: from prefix 0; a prefix-1 entry matches its exact
	// address, ends the walk and overrides what was found before it
	int32_t abest = 0;
	uint32_t aidx = 0xFFFFu;
	if (walk) {
		for (uint32_t j = 0; j < nr; j++) {
			const int32_t pf = s_rp[j];
			if ((daddr & s_rm[j]) == s_rv[j] && pf > best) {
				best = pf;
				nif = s_rn[j];
			}
		}
		bool done = false;
		for (uint32_t j = 0; j < na; j++) {
			const int32_t pf = s_ap[j];
			const bool m = (daddr & s_am[j]) == s_av[j];
			const bool take = !done && m && (pf == 1 || pf > abest);
			if (take) {
				aidx = j;
				abest = pf == 1 ? abest : pf;
				done = pf == 1;
			}
		}
	}
	uint32_t kind = MOSRX_FWD_NONE, tx_len = 0, arp = 0xFFFFu;
	int32_t oif = -1;
	if (fwd && eth && cap >= 14u) {
		if (nicout == -1)
			kind = MOSRX_FWD_NO_NIC;
		else {
			kind = MOSRX_FWD_ETH;
			tx_len = cap;
			oif = nicout;
		}
	} else if (fwd && !eth && ip_ok) {
		if (!walk) {
			kind = MOSRX_FWD_IP;
			oif = nicout;
		} else if (nif < 0)
			kind = MOSRX_FWD_NO_ROUTE;
		else if (aidx == 0xFFFFu) {
			kind = MOSRX_FWD_NO_ARP;
			oif = nif;
		} else {
			kind = MOSRX_FWD_IP;
			oif = nif;
			arp = aidx;
		}
		if (kind == MOSRX_FWD_IP)
			tx_len = 14u + ip_len;
	}
	u32x2 v;
	v.x = tx_len | (((uint32_t)oif & 0xFFu) << 16) | (kind << 24);
	v.y = arp;
#else
#error "FWD_PLAN: 1 tables, 2 record"
#endif
#undef FWD_PLAN
