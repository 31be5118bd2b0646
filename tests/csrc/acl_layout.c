/* Prints the layout of the firewall rule record and of the launch's
 * parameters, one "name value" per line (tests/test_acl.py compares it with the
 * Python mirrors and the sizes the headers assert). */
#include <stddef.h>
#include <stdio.h>

#include "mosrx_acl.h"

#define SZ(t) printf("sizeof(" #t ") %zu\n", sizeof(t))
#define OFF(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))

int main(void)
{
	SZ(mosrx_acl_rule);
	OFF(mosrx_acl_rule, src_ip);
	OFF(mosrx_acl_rule, src_mask);
	OFF(mosrx_acl_rule, dst_ip);
	OFF(mosrx_acl_rule, dst_mask);
	OFF(mosrx_acl_rule, sport);
	OFF(mosrx_acl_rule, dport);
	OFF(mosrx_acl_rule, action);
	OFF(mosrx_acl_rule, pad);
	SZ(mosrx_adesc);
	SZ(mosrx_aparams);
	OFF(mosrx_aparams, frames);
	OFF(mosrx_aparams, off);
	OFF(mosrx_aparams, len);
	OFF(mosrx_aparams, rec);
	OFF(mosrx_aparams, plan);
	OFF(mosrx_aparams, hit);
	OFF(mosrx_aparams, adesc);
	OFF(mosrx_aparams, fdesc);
	OFF(mosrx_aparams, tab);
	OFF(mosrx_aparams, counts);
	OFF(mosrx_aparams, frames_bytes);
	OFF(mosrx_aparams, n);
	OFF(mosrx_aparams, nb);
	OFF(mosrx_aparams, total_tiles);
	OFF(mosrx_aparams, rec_bytes);
	OFF(mosrx_aparams, forward);
	OFF(mosrx_aparams, num_msp);
	OFF(mosrx_aparams, listener);
	SZ(mosrx_acl_dev);
	SZ(mosrx_fwd);
	printf("MOSRX_ACL_MAX_RULES %d\n", MOSRX_ACL_MAX_RULES);
	printf("MOSRX_ACL_ACCEPT %d\n", MOSRX_ACL_ACCEPT);
	printf("MOSRX_ACL_DROP %d\n", MOSRX_ACL_DROP);
	printf("MOSRX_FWD_DROP %d\n", MOSRX_FWD_DROP);
	printf("MOSRX_ACL_NOT_LOOKED_UP %u\n", MOSRX_ACL_NOT_LOOKED_UP);
	printf("MOSRX_ACL_NO_MATCH %u\n", MOSRX_ACL_NO_MATCH);
	printf("MOSRX_ACL_TILE %u\n", MOSRX_ACL_TILE);
	printf("MOSRX_OP_ACL %d\n", MOSRX_OP_ACL);
	return 0;
}
