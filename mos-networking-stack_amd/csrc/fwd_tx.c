/*
 * fwd_tx.c — the host half of "the TX run handed to send_pkts": the per-netdev
 * rings mosrx_fwd_build_rings_dev built, copied back, go to an io_module_func
 * as mOS itself transmits -- get_wptr(ctx, nif, len) per frame, one
 * send_pkts(ctx, nif) per netdev at the end of the round (core.c:999-1007).
 * Plain C, no GPU call.
 */
#include <errno.h>
#include <string.h>

#include "../../include/mosrx_io_module.h"

int mosrx_fwd_rings_send(const io_module_func *iom, struct mtcp_thread_context *ctx, const uint8_t *h_tx_frames,
                         const uint32_t *h_tx_off, const uint16_t *h_tx_len, const mosrx_fwd_ring *h_rings,
                         uint32_t nrings, mosrx_fwd_send_stats *st)
{
	uint64_t sent = 0, no_buffer = 0, calls = 0;
	uint32_t q, r;
	if (!iom || !iom->get_wptr || !iom->send_pkts || !ctx || !h_tx_frames || !h_tx_off || !h_tx_len || !h_rings ||
	    nrings < 1 || nrings > MOSRX_FWD_MAX_NETDEVS)
		return -EINVAL;
	for (q = 0; q < nrings; q++) {
		const uint32_t start = h_rings[q].start, count = h_rings[q].count;
		if (!count)
			continue;
		for (r = 0; r < count; r++) {
			const uint16_t len = h_tx_len[start + r];
			uint8_t *w = iom->get_wptr(ctx, (int)q, len);
			if (!w) {
				no_buffer++;   /* EthernetOutput returned NULL: the frame is lost, the next one is tried */
				continue;
			}
			memcpy(w, h_tx_frames + h_tx_off[start + r], len);
			sent++;
		}
		iom->send_pkts(ctx, (int)q);
		calls++;
	}
	if (st) {
		st->sent += sent;
		st->no_buffer += no_buffer;
		st->send_calls += calls;
	}
	return (int)sent;
}
