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

/* The same hand-over from the descriptor form (mosrx_fwd_desc_rings_dev): the
 * frames never left the host, so each is copied from where it was received and
 * its 12 address bytes laid over the start.  Reads entries start .. start +
 * count of each ring and nothing else. */
int mosrx_fwd_desc_send(const io_module_func *iom, struct mtcp_thread_context *ctx, const uint8_t *frames,
                        const uint32_t *off, const uint32_t *h_tx_src, const uint16_t *h_tx_len,
                        const uint32_t *h_tx_mac, const mosrx_fwd_ring *h_rings, uint32_t nrings,
                        mosrx_fwd_send_stats *st)
{
	uint64_t sent = 0, no_buffer = 0, calls = 0;
	uint32_t q, r;
	if (!iom || !iom->get_wptr || !iom->send_pkts || !ctx || !frames || !off || !h_tx_src || !h_tx_len || !h_tx_mac ||
	    !h_rings || nrings < 1 || nrings > MOSRX_FWD_MAX_NETDEVS)
		return -EINVAL;
	for (q = 0; q < nrings; q++) {
		const uint32_t start = h_rings[q].start, count = h_rings[q].count;
		if (!count)
			continue;
		for (r = 0; r < count; r++) {
			const uint32_t e = start + r;
			const uint16_t len = h_tx_len[e];
			uint8_t *w = iom->get_wptr(ctx, (int)q, len);
			if (!w) {
				no_buffer++;   /* as mosrx_fwd_rings_send: the frame is lost, the next one is tried */
				continue;
			}
			memcpy(w, frames + off[h_tx_src[e]], len);
			memcpy(w, h_tx_mac + 3u * (size_t)e, len < 12 ? len : 12);   /* (a sent frame has len >= 14) */
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

int mosrx_backend_forward(const io_module_func *iom, struct mtcp_thread_context *ctx, int ifidx,
                          mosrx_fwd_send_stats *st)
{
	mosrx_fwd_view v;
	uint64_t total = 0;
	uint32_t q, r;
	if (!iom || !iom->dev_ioctl || !ctx)
		return -EINVAL;
	memset(&v, 0, sizeof(v));
	if (iom->dev_ioctl(ctx, ifidx, MOSRX_PKT_RX_FWD, &v))
		return -1;
	if (v.nrings < 1 || v.nrings > MOSRX_FWD_MAX_NETDEVS || !v.rings || !v.tx_src)
		return -EIO;
	/* the view carries n: every entry names a frame of the batch */
	for (q = 0; q < v.nrings; q++) {
		total += v.rings[q].count;
		if ((uint64_t)v.rings[q].start + v.rings[q].count > v.n)
			return -EIO;
		for (r = 0; r < v.rings[q].count; r++)
			if (v.tx_src[v.rings[q].start + r] >= v.n)
				return -EIO;
	}
	if (total > v.n)
		return -EIO;
	return mosrx_fwd_desc_send(iom, ctx, v.frames, v.off, v.tx_src, v.tx_len, v.tx_mac, v.rings, v.nrings, st);
}
