// mosrx_fwd_desc_entry.inc — one sent frame's descriptor entry, included into the
// store launch's body (fwd_desc_store_body) and into the one-launch kernel
// (mosrx_fwd.hip); text for the reason mosrx_fwd_rings_body.inc gives.  In scope:
//   p       a mosrx_dparams: frames, frames_bytes, tab, tx_src, tx_len, tx_mac
//   i, o    the frame and its offset;  pl its plan record;  q its netdev (< nrings)
//   j       its entry (< p.n)
		// bytes 0 .. 11 of the frame the byte-ring copy writes (its r == 0 unit)
		const __amdgpu_buffer_rsrc_t rs = frame_rsrc(p.frames, p.frames_bytes);
		const mosrx_fwd_dev *T = p.tab;
		const u32x4 h = fwd_ld128(rs, o);
		u32x3 m = {h.x, h.y, h.z};
		if ((pl.x >> 24) == MOSRX_FWD_IP) {
			const uint32_t ai = pl.y & 0xFFFFu;
			const uint32_t nif = q & (MOSRX_FWD_MAX_NETDEVS - 1u);
			const uint32_t *sm = reinterpret_cast<const uint32_t *>(T->netdev_haddr[nif]);
			const uint32_t s0 = sm[0], s1 = sm[1] & 0xFFFFu;
			uint32_t d0 = h.x, d1 = h.y & 0xFFFFu;   // the frame's own h_dest (nic_forward_table path)
			if (ai < MOSRX_FWD_MAX_ARP) {
				const uint32_t *dm = reinterpret_cast<const uint32_t *>(T->a_haddr[ai]);
				d0 = dm[0];
				d1 = dm[1] & 0xFFFFu;
			}
			m.x = d0;
			m.y = d1 | (s0 << 16);
			m.z = (s0 >> 16) | (s1 << 16);
		}
		p.tx_src[j] = i;
		p.tx_len[j] = (uint16_t)(pl.x & 0xFFFFu);
		uint32_t *mac = p.tx_mac + 3u * (uint64_t)j;
		mac[0] = m.x;
		mac[1] = m.y;
		mac[2] = m.z;
