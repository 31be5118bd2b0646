/* Prints the layout facts tests/test_steer_one.py pins: the steer descriptors'
 * sizes, where mosrx_sparams.fused sits, the cap, and the configuration struct
 * (which the one-launch setting must not have changed). */
#include <stddef.h>
#include <stdio.h>

#include "mosrx_io_module.h"
#include "mosrx_steer.h"

int main(void)
{
	printf("%zu %zu %zu %zu %zu %zu %u %zu %zu %zu\n", sizeof(mosrx_sdesc), sizeof(mosrx_gdesc), sizeof(mosrx_xdesc),
	       sizeof(mosrx_sparams), offsetof(mosrx_sparams, side), offsetof(mosrx_sparams, fused), MOSRX_STEER_ONE_MAX,
	       sizeof(mosrx_gpu_module_cfg), offsetof(mosrx_gpu_module_cfg, steer),
	       offsetof(mosrx_gpu_module_cfg, direct_frames));
	return 0;
}
