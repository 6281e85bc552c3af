// block_rescale_packed_limit.hip -- motion -b with -s AND --coeff-limit on packed 8-bit pixels (dspfft_execute_roundtrip_u8_packed_rescale_limit):
// block_rs_packed_wide_core.h's sequence with the selection and the plain packed store, one kernel per number of components.  A unit of its own:
// block_rescale_packed.hip's build and code objects stay what they were.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rs_packed_wide_core.h"

/* rt_run_packed_grid's launch when the call carries a coefficient limit and no -d (engine.cpp reaches this through a weak reference: the CPU
 * emulation links engine.cpp without this unit).  lds: the tile's bytes; the tables and the counter follow it.  -1: extents, a number of components
 * or an embedding without a kernel, a tile that does not fit, or a limit that is none (0, or the whole embedding). */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_rescale_packed_limit_launch(const dspfft::BlockRsPackedWideArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockRsPackedWideArgs &a = *ap;
	if (!a.keep || a.dither) return -1;
	lds = rs_packed_wide_lds(a, nwg, lds);
	if (!lds) return -1;
	switch (a.comps) {
	case 2: return launch_block_rescale_packed_wide<2, true, false>(a, nwg, lds, stream);
	case 3: return launch_block_rescale_packed_wide<3, true, false>(a, nwg, lds, stream);
	case 4: return launch_block_rescale_packed_wide<4, true, false>(a, nwg, lds, stream);
	}
	return -1;
}
