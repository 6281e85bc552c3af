// block_rescale_packed_dither.hip -- motion -b with -s AND -d on packed 8-bit pixels, with or without --coeff-limit
// (dspfft_execute_roundtrip_u8_packed_rescale_dither): block_rs_packed_wide_core.h's sequence with the Floyd-Steinberg store in the tile, one kernel
// per number of components and per kind of middle (fused, or unfused around the selection).
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rs_packed_wide_core.h"

/* rt_run_packed_grid's launch for a dithered call (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without
 * this unit).  lds: the tile's bytes; the tables, the counter, the dither's table and its error rows follow it.  -1: extents, a number of
 * components or an embedding without a kernel, or the whole does not fit. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_rescale_packed_dither_launch(const dspfft::BlockRsPackedWideArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockRsPackedWideArgs &a = *ap;
	if (!a.dither) return -1;
	lds = rs_packed_wide_lds(a, nwg, lds);
	if (!lds) return -1;
	switch (a.comps * 2 + (a.keep ? 1 : 0)) {
	case 4: return launch_block_rescale_packed_wide<2, false, true>(a, nwg, lds, stream);
	case 5: return launch_block_rescale_packed_wide<2, true, true>(a, nwg, lds, stream);
	case 6: return launch_block_rescale_packed_wide<3, false, true>(a, nwg, lds, stream);
	case 7: return launch_block_rescale_packed_wide<3, true, true>(a, nwg, lds, stream);
	case 8: return launch_block_rescale_packed_wide<4, false, true>(a, nwg, lds, stream);
	case 9: return launch_block_rescale_packed_wide<4, true, true>(a, nwg, lds, stream);
	}
	return -1;
}
