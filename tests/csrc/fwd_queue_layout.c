/* Prints the layout of the batch-queue forwarding structures, one
 * "name value" per line (tests/test_fwd_queue.py compares it with the Python
 * mirror and the sizes the header asserts). */
#include <stddef.h>
#include <stdio.h>

#include "mosrx_fwd.h"

#define SZ(t) printf("sizeof(" #t ") %zu\n", sizeof(t))
#define OFF(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))

int main(void)
{
	SZ(mosrx_queue_fwd);
	OFF(mosrx_queue_fwd, in_ifidx);
	OFF(mosrx_queue_fwd, d_plan);
	OFF(mosrx_queue_fwd, ring_cap);
	OFF(mosrx_queue_fwd, nrings);
	OFF(mosrx_queue_fwd, d_tx_frames);
	OFF(mosrx_queue_fwd, d_tx_off);
	OFF(mosrx_queue_fwd, d_tx_len);
	OFF(mosrx_queue_fwd, d_tx_src);
	OFF(mosrx_queue_fwd, d_rings);
	SZ(mosrx_fdesc);
	OFF(mosrx_fdesc, frames);
	OFF(mosrx_fdesc, off);
	OFF(mosrx_fdesc, len);
	OFF(mosrx_fdesc, rec);
	OFF(mosrx_fdesc, plan);
	OFF(mosrx_fdesc, tx);
	OFF(mosrx_fdesc, tx_off);
	OFF(mosrx_fdesc, tx_len);
	OFF(mosrx_fdesc, tx_src);
	OFF(mosrx_fdesc, rings);
	OFF(mosrx_fdesc, frames_bytes);
	OFF(mosrx_fdesc, n);
	OFF(mosrx_fdesc, in_ifidx);
	OFF(mosrx_fdesc, tile_base);
	SZ(mosrx_fqparams);
	OFF(mosrx_fqparams, desc);
	OFF(mosrx_fqparams, tab);
	OFF(mosrx_fqparams, scratch);
	OFF(mosrx_fqparams, nb);
	OFF(mosrx_fqparams, total_tiles);
	OFF(mosrx_fqparams, rec_bytes);
	OFF(mosrx_fqparams, forward);
	OFF(mosrx_fqparams, num_msp);
	OFF(mosrx_fqparams, listener);
	OFF(mosrx_fqparams, nrings);
	OFF(mosrx_fqparams, cap_units);
	return 0;
}
