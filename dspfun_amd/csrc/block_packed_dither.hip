// block_packed_dither.hip -- motion -d on packed small blocks (dspfft_execute_roundtrip_u8_packed_dither): block_packed_rt.h's two sequences on
// BlockPackedDitherArgs -- the Floyd-Steinberg store runs in the LDS tile (block_packed_core.h) and the bytes leave through the packed store --
// over DSPFFT_BLOCK_SHAPES x C in {2, 3, 4}, and their dispatch.  A unit of its own: block_packed.hip's build and code objects stay what they were.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_packed_rt.h"

namespace dspfft {

template <int NX, int NY, int NZ, int C, bool TOPN>
static int launch_block_packed_dither(const BlockPackedDitherArgs &a, int nwg, size_t lds, void *stream)
{
	const auto kern = TOPN ? &block_packed_topn_kernel<NX, NY, NZ, C, BlockPackedDitherArgs> : &block_packed_kernel<NX, NY, NZ, C, BlockPackedDitherArgs>;
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL(kern, dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}

template <int NX, int NY, int NZ>
static int launch_block_packed_dither_c(const BlockPackedDitherArgs &a, int nwg, size_t lds, void *stream)
{
	switch (a.comps * 2 + (a.keep ? 1 : 0)) {
	case 4: return launch_block_packed_dither<NX, NY, NZ, 2, false>(a, nwg, lds, stream);
	case 5: return launch_block_packed_dither<NX, NY, NZ, 2, true>(a, nwg, lds, stream);
	case 6: return launch_block_packed_dither<NX, NY, NZ, 3, false>(a, nwg, lds, stream);
	case 7: return launch_block_packed_dither<NX, NY, NZ, 3, true>(a, nwg, lds, stream);
	case 8: return launch_block_packed_dither<NX, NY, NZ, 4, false>(a, nwg, lds, stream);
	case 9: return launch_block_packed_dither<NX, NY, NZ, 4, true>(a, nwg, lds, stream);
	}
	return -1;
}

}  // namespace dspfft

/* dspfft_execute_roundtrip_u8_packed_dither's launch (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without
 * this unit).  lds: the tile's bytes; the transfer tables follow it when the call has any, then the dither phase's table and error rows
 * (packed_dither_bytes of a.slots).  -1: no kernel for these block extents or this number of components, or the whole does not fit. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_packed_dither_launch(const dspfft::BlockPackedDitherArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockPackedDitherArgs &a = *ap;
	if (!a.in8 || !a.out8 || (lds & 15) || a.slots != packed_dither_slots(a.nz, a.comps, a.G)) return -1;
	if (a.tab_in || a.tab_out) lds += sizeof(TrcU8Tab);
	lds += packed_dither_bytes(a.nx, a.slots);
	if (lds + 16 > 64 * 1024) return -1;
#define DSP_BLOCK_CASE(X_, Y_, Z_) \
	if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) return launch_block_packed_dither_c<X_, Y_, Z_>(a, nwg, lds, stream);
	DSPFFT_BLOCK_SHAPES(DSP_BLOCK_CASE)
#undef DSP_BLOCK_CASE
	return -1;
}
