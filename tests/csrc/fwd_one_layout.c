/* Prints the layout of the one-launch forwarding form's parameters, one
 * "name value" per line (tests/test_fwd_one.py compares it with the Python
 * mirror and the sizes the header asserts). */
#include <stddef.h>
#include <stdio.h>

#include "mosrx_fwd.h"

#define SZ(t) printf("sizeof(" #t ") %zu\n", sizeof(t))
#define OFF(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))

int main(void)
{
	SZ(mosrx_oparams);
	OFF(mosrx_oparams, fdesc);
	OFF(mosrx_oparams, ddesc);
	OFF(mosrx_oparams, tab);
	OFF(mosrx_oparams, nb);
	OFF(mosrx_oparams, rec_bytes);
	OFF(mosrx_oparams, forward);
	OFF(mosrx_oparams, num_msp);
	OFF(mosrx_oparams, listener);
	OFF(mosrx_oparams, nrings);
	OFF(mosrx_oparams, onef);
	OFF(mosrx_oparams, oned);
	SZ(mosrx_fdesc);
	SZ(mosrx_fqparams);
	SZ(mosrx_ddesc);
	OFF(mosrx_ddesc, frames);
	OFF(mosrx_ddesc, off);
	OFF(mosrx_ddesc, plan);
	OFF(mosrx_ddesc, tx_src);
	OFF(mosrx_ddesc, tx_len);
	OFF(mosrx_ddesc, tx_mac);
	OFF(mosrx_ddesc, rings);
	OFF(mosrx_ddesc, frames_bytes);
	OFF(mosrx_ddesc, n);
	OFF(mosrx_ddesc, tile_base);
	OFF(mosrx_ddesc, pad);
	SZ(mosrx_dqparams);
	printf("MOSRX_FWD_ONE_MAX %u\n", MOSRX_FWD_ONE_MAX);
	printf("MOSRX_FWD_TILE %u\n", MOSRX_FWD_TILE);
	return 0;
}
