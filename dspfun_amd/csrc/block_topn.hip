// block_topn.hip -- the fused small-block roundtrip with motion's --coeff-limit (motion/motion.c:652-668) between the forward transform and
// the filter: block_rt.h's block_roundtrip_topn_kernel on float and plain 8-bit ends, and its dispatch.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rt.h"

namespace dspfft {

template <int NX, int NY, int NZ, bool IN8, bool OUT8>
static int launch_block_rt_topn(const BlockRtTopnArgs &a, int nwg, size_t lds, void *stream)
{
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_roundtrip_topn_kernel<NX, NY, NZ, IN8, OUT8, BlockRtTopnArgs>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL((block_roundtrip_topn_kernel<NX, NY, NZ, IN8, OUT8, BlockRtTopnArgs>), dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}

}  // namespace dspfft

/* rt_run_block's launch when the call carries a coefficient limit (engine.cpp reaches this through a weak reference: the CPU emulation of the
 * kernel phases links engine.cpp without this unit).  -1: no kernel for these block extents. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_topn_launch(const dspfft::BlockRtTopnArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockRtTopnArgs &a = *ap;
#define DSP_BLOCK_CASE(X_, Y_, Z_) \
	if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) { \
		if (a.in8) return a.out8 ? launch_block_rt_topn<X_, Y_, Z_, true, true>(a, nwg, lds, stream) : launch_block_rt_topn<X_, Y_, Z_, true, false>(a, nwg, lds, stream); \
		return a.out8 ? launch_block_rt_topn<X_, Y_, Z_, false, true>(a, nwg, lds, stream) : launch_block_rt_topn<X_, Y_, Z_, false, false>(a, nwg, lds, stream); \
	}
	DSPFFT_BLOCK_SHAPES(DSP_BLOCK_CASE)
#undef DSP_BLOCK_CASE
	return -1;
}
