// block_trc.hip -- the fused small-block roundtrip of 8-bit video with motion --linear (dspfft_plan_set_u8_trc): block_rt.h's two kernels
// on BlockRtTrcArgs, with the transfer characteristic's decode table at the load and its threshold table at the store, both in LDS behind
// the tile (3 KB), and their dispatch.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rt.h"

namespace dspfft {

// OUT8 = false: the dithered roundtrip, whose bytes the dither kernel stores from the float result (with a coefficient limit:
// dspfft_execute_roundtrip_u8_dither_limit)
template <int NX, int NY, int NZ, bool OUT8, bool TOPN>
static auto block_trc_kernel()
{
	if constexpr (TOPN) return &block_roundtrip_topn_kernel<NX, NY, NZ, true, OUT8, BlockRtTrcArgs>;
	else return &block_roundtrip_kernel<NX, NY, NZ, true, OUT8, BlockRtTrcArgs>;
}

template <int NX, int NY, int NZ, bool OUT8, bool TOPN>
static int launch_block_rt_trc(const BlockRtTrcArgs &a, int nwg, size_t lds, void *stream)
{
	const auto kern = block_trc_kernel<NX, NY, NZ, OUT8, TOPN>();
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL(kern, dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}

}  // namespace dspfft

/* rt_run_block's launch when an 8-bit end has a transfer characteristic (engine.cpp reaches this through a weak reference).  lds: the tile's
 * bytes; the tables follow it.  a.keep = 0: no coefficient limit.  -1: no kernel for these block extents, or the tables do not fit. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_trc_launch(const dspfft::BlockRtTrcArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockRtTrcArgs &a = *ap;
	if (!a.in8 || (lds & 15) || lds + sizeof(TrcU8Tab) > 64 * 1024) return -1;
	lds += sizeof(TrcU8Tab);
#define DSP_BLOCK_CASE(X_, Y_, Z_) \
	if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { \
		if (a.keep) return a.out8 ? launch_block_rt_trc<X_, Y_, Z_, true, true>(a, nwg, lds, stream) : launch_block_rt_trc<X_, Y_, Z_, false, true>(a, nwg, lds, stream); \
		return a.out8 ? launch_block_rt_trc<X_, Y_, Z_, true, false>(a, nwg, lds, stream) : launch_block_rt_trc<X_, Y_, Z_, false, false>(a, nwg, lds, stream); \
	}
	DSPFFT_BLOCK_SHAPES(DSP_BLOCK_CASE)
#undef DSP_BLOCK_CASE
	return -1;
}
