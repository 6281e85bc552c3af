// block_packed.hip -- the fused small-block roundtrip on packed 8-bit pixels (rgb24, rgba ...: dspfft_execute_roundtrip_u8_packed): block_packed_rt.h's two
// sequences of phases, the plain one and the one with motion --coeff-limit's selection, with block_packed_core.h's ends and per-component filter,
// over DSPFFT_BLOCK_SHAPES x C in {2, 3, 4}, and their dispatch.  One argument structure: the tables of motion --linear are staged in LDS behind the
// tile when the call has any (a NULL pointer: that end converts plainly).
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_packed_rt.h"

namespace dspfft {

template <int NX, int NY, int NZ, int C, bool TOPN>
static int launch_block_packed(const BlockPackedArgs &a, int nwg, size_t lds, void *stream)
{
	const auto kern = TOPN ? &block_packed_topn_kernel<NX, NY, NZ, C, BlockPackedArgs> : &block_packed_kernel<NX, NY, NZ, C, BlockPackedArgs>;
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL(kern, dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}

template <int NX, int NY, int NZ>
static int launch_block_packed_c(const BlockPackedArgs &a, int nwg, size_t lds, void *stream)
{
	switch (a.comps * 2 + (a.keep ? 1 : 0)) {
	case 4: return launch_block_packed<NX, NY, NZ, 2, false>(a, nwg, lds, stream);
	case 5: return launch_block_packed<NX, NY, NZ, 2, true>(a, nwg, lds, stream);
	case 6: return launch_block_packed<NX, NY, NZ, 3, false>(a, nwg, lds, stream);
	case 7: return launch_block_packed<NX, NY, NZ, 3, true>(a, nwg, lds, stream);
	case 8: return launch_block_packed<NX, NY, NZ, 4, false>(a, nwg, lds, stream);
	case 9: return launch_block_packed<NX, NY, NZ, 4, true>(a, nwg, lds, stream);
	}
	return -1;
}

}  // namespace dspfft

/* dspfft_execute_roundtrip_u8_packed's launch (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without this
 * unit).  lds: the tile's bytes; the tables follow it when the call has any.  a.keep = 0: no coefficient limit.  -1: no kernel for these block
 * extents or this number of components, or tile and tables do not fit. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_packed_launch(const dspfft::BlockPackedArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockPackedArgs &a = *ap;
	if (!a.in8 || !a.out8 || (lds & 15)) return -1;
	if (a.tab_in || a.tab_out) lds += sizeof(TrcU8Tab);
	if (lds + 16 > 64 * 1024) return -1;
#define DSP_BLOCK_CASE(X_, Y_, Z_) \
	if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) return launch_block_packed_c<X_, Y_, Z_>(a, nwg, lds, stream);
	DSPFFT_BLOCK_SHAPES(DSP_BLOCK_CASE)
#undef DSP_BLOCK_CASE
	return -1;
}
