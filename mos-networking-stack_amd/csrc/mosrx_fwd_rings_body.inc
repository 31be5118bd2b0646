// mosrx_fwd_rings_body.inc — the bodies of the ring build's three launches,
// included into the single-batch kernels and into their batch-queue forms
// (mosrx_fwd.hip).  Text, not functions: a call boundary, even one inlined away,
// changes the code the compiler makes for the single-batch kernels (operand
// and load order, scheduling), and those are pinned against their earlier
// disassembly.  In scope at the include:
//   p         a mosrx_rparams: the batch, its outputs and its scratch rows
//   FWD_BODY  1 totals, 2 scan, 3 copy
//   FWD_BLK   (totals, copy) the workgroup's tile within the batch
//   FWD_SKIP  (scan) true for a workgroup that has no batch
#if FWD_BODY == 1
	__shared__ uint32_t s_wu[FWD_WAVES][FWD_NQ], s_wc[FWD_WAVES][FWD_NQ];
	if (FWD_BLK >= p.tiles)
		return;
	const uint32_t nrings = min(p.nrings, FWD_NQ);
	const uint32_t t = threadIdx.x, i = FWD_BLK * MOSRX_FWD_TILE + t;
	u32x2 pl = {0u, 0u};
	if (i < p.n)
		pl = *reinterpret_cast<const u32x2 *>(p.plan + i);
	uint32_t q, excl, rank;
	const uint32_t units = fwd_ring_units(pl, nrings, q);
	fwd_ring_tile_scan(q, units, nrings, s_wu, s_wc, excl, rank);
	if (t < nrings) {
		uint32_t tu = 0, tc = 0;
#pragma unroll
		for (uint32_t w = 0; w < FWD_WAVES; w++) {
			tu += s_wu[w][t];
			tc += s_wc[w][t];
		}
		u32x4 row = {tu, tc, 0u, 0u};
		*reinterpret_cast<u32x4 *>(p.scratch + 4u * ((uint64_t)FWD_BLK * nrings + t)) = row;
	}
#elif FWD_BODY == 2
	__shared__ uint32_t s_tot[FWD_NQ];
	static_assert(FWD_SCAN_THREADS / 64u == FWD_NQ, "one wave per netdev");
	if (FWD_SKIP)
		return;
	const uint32_t nrings = min(p.nrings, FWD_NQ);
	const uint32_t t = threadIdx.x, lane = t & 63u, q = t >> 6;
	const uint32_t per = (p.tiles + 63u) / 64u;
	const uint32_t t0 = min(lane * per, p.tiles), t1 = min(t0 + per, p.tiles);
	const bool col = q < nrings;
	uint64_t su = 0;
	uint32_t sc = 0;
	if (col)
		for (uint32_t r = t0; r < t1; r++) {
			const uint32_t *row = p.scratch + 4u * ((uint64_t)r * nrings + q);
			su += row[0];
			sc += row[1];
		}
	// inclusive prefix over the wave's 64 runs
	uint64_t iu = su;
	uint32_t ic = sc;
#pragma unroll
	for (uint32_t o = 1; o < 64u; o <<= 1) {
		const uint32_t xl = __shfl_up((uint32_t)iu, o), xh = __shfl_up((uint32_t)(iu >> 32), o);
		const uint32_t xc = __shfl_up(ic, o);
		iu += lane >= o ? ((uint64_t)xl | ((uint64_t)xh << 32)) : 0u;
		ic += lane >= o ? xc : 0u;
	}
	if (lane == 63u)
		s_tot[q] = col ? ic : 0u;
	__syncthreads();
	if (!col)
		return;
	uint32_t start = 0;
	for (uint32_t g = 0; g < nrings; g++)
		start += g < q ? s_tot[g] : 0u;
	uint64_t ru = iu - su;
	uint32_t rc = start + ic - sc;
	for (uint32_t r = t0; r < t1; r++) {
		uint32_t *row = p.scratch + 4u * ((uint64_t)r * nrings + q);
		const uint32_t u = row[0], c = row[1];
		u32x4 v = {(uint32_t)ru, (uint32_t)(ru >> 32), rc, 0u};
		*reinterpret_cast<u32x4 *>(row) = v;
		ru += u;
		rc += c;
	}
	if (lane == 0u) {
		u32x4 v = {start, 0u, 0u, 0u};
		*reinterpret_cast<u32x4 *>(p.rings + q) = v;
	}
#elif FWD_BODY == 3
	__shared__ uint32_t s_wu[FWD_WAVES][FWD_NQ], s_wc[FWD_WAVES][FWD_NQ];
	__shared__ uint32_t s_nf[FWD_WAVES][FWD_NQ], s_nd[FWD_WAVES][FWD_NQ], s_end[FWD_WAVES][FWD_NQ];
	__shared__ uint32_t s_au[FWD_WAVES], s_ac[FWD_WAVES];
	__shared__ uint32_t s_start[MOSRX_FWD_TILE + 1u];   // unit start, among the tile's written units, of its k-th written frame
	__shared__ uint32_t s_dst[MOSRX_FWD_TILE];          // its first unit in tx
	__shared__ uint32_t s_off[MOSRX_FWD_TILE];          // its source offset
	__shared__ uint32_t s_meta[MOSRX_FWD_TILE];         // its plan word 0 (tx_len, out_ifidx, kind)
	__shared__ uint32_t s_arp[MOSRX_FWD_TILE];
	if (FWD_BLK >= p.tiles)
		return;
	const uint32_t nrings = min(p.nrings, FWD_NQ);
	const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, i = FWD_BLK * MOSRX_FWD_TILE + t;
	u32x2 pl = {0u, 0u};
	uint32_t o = 0;
	if (i < p.n) {
		pl = *reinterpret_cast<const u32x2 *>(p.plan + i);
		o = p.off[i];
	}
	uint32_t q, excl, rank;
	const uint32_t units = fwd_ring_units(pl, nrings, q);
	const bool sent = units != 0u;
	fwd_ring_tile_scan(q, units, nrings, s_wu, s_wc, excl, rank);
	u32x4 row = {0u, 0u, 0u, 0u};
	if (sent)
		row = *reinterpret_cast<const u32x4 *>(p.scratch + 4u * ((uint64_t)FWD_BLK * nrings + q));
	const uint64_t k = ((uint64_t)row.x | ((uint64_t)row.y << 32)) + excl;
	const uint32_t j = row.z + rank;
	// written: the frame fits its ring and has an entry
	const bool live = sent && k + units <= (uint64_t)p.cap_units && j < p.n;
	const uint32_t k32 = live ? (uint32_t)k : 0u;
	const uint32_t dst0 = q * p.cap_units + k32;      // < nrings * cap_units <= 2^28
	if (live) {
		p.tx_off[j] = dst0 * 16u + 2u;
		p.tx_len[j] = (uint16_t)(pl.x & 0xFFFFu);
		p.tx_src[j] = i;
	}
	// the wave's share of count / dropped / units per ring
	for (uint32_t g = 0; g < nrings; g++) {
		const uint64_t fm = __ballot(live && q == g);
		const uint64_t dm = __ballot(sent && !live && q == g);
		// the ring's last written frame in this wave ends the ring's filled part
		const uint32_t last = fm ? 63u - (uint32_t)__builtin_clzll(fm) : 0u;
		const uint32_t end = __builtin_amdgcn_readlane(k32 + units, last);
		if (lane == 0u) {
			s_nf[wave][g] = (uint32_t)__builtin_popcountll(fm);
			s_nd[wave][g] = (uint32_t)__builtin_popcountll(dm);
			s_end[wave][g] = fm ? end : 0u;
		}
	}
	// the tile's written units in arrival order, for dealing them to the lanes
	uint32_t aexcl, arank, tu, ts;
	fwd_tile_scan(live ? units : 0u, s_au, s_ac, aexcl, arank, tu, ts);
	if (live) {
		s_start[arank] = aexcl;
		s_dst[arank] = dst0;
		s_off[arank] = o;
		s_meta[arank] = pl.x;
		s_arp[arank] = pl.y & 0xFFFFu;
	}
	if (t == 0)
		s_start[ts] = tu;
	__syncthreads();
	if (t < nrings) {
		uint32_t nf = 0, nd = 0, end = 0;
#pragma unroll
		for (uint32_t w = 0; w < FWD_WAVES; w++) {
			nf += s_nf[w][t];
			nd += s_nd[w][t];
			end = max(end, s_end[w][t]);
		}
		mosrx_fwd_ring *rg = p.rings + t;
		if (nf) {
			atomicAdd(&rg->count, nf);
			atomicMax(&rg->units, end);
		}
		if (nd)
			atomicAdd(&rg->dropped, nd);
	}
	const __amdgpu_buffer_rsrc_t rs = frame_rsrc(p.frames, p.frames_bytes);
	const mosrx_fwd_dev *T = p.tab;
	const uint32_t tx_units = nrings * p.cap_units;
	for (uint32_t u = t; u < tu; u += MOSRX_FWD_THREADS) {
		// the written frame that holds unit u: the last one starting at or before it
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
		const uint32_t r = u - s_start[lo];
		const uint32_t tx_len = meta & 0xFFFFu;
		const uint32_t du = s_dst[lo] + r;
		if (du >= tx_units || 16u * r >= tx_len + 2u)
			continue;                      // (holds by construction: the frame's last unit fits its ring)
		uint8_t *dst = p.tx + (uint64_t)du * 16u;
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
				for (uint32_t g = 0; g < 4u; g++) {
					if (g < nd)
						reinterpret_cast<uint32_t *>(dst)[g] = w[g];
					last = g == nd ? w[g] : last;
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
#else
#error "FWD_BODY: 1 totals, 2 scan, 3 copy"
#endif
#undef FWD_BODY
#undef FWD_BLK
#undef FWD_SKIP
