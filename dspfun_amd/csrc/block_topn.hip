// block_topn.hip -- the fused small-block roundtrip with motion's --coeff-limit (motion/motion.c:652-668) between the forward transform and
// the filter: block_roundtrip_kernel's load, store and helpers (block_core.h) with the middle unfused, because the selection needs the whole
// block's coefficients before any of them is filtered.  A translation unit of its own: it compiles beside block_fused.hip, which is unchanged.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "topn_core.h"

namespace dspfft {

// load (float / 8-bit), REDFT10 along x, y, z | per-block top-N (topn_core.h) | filter | REDFT01 along z, y, x, store
template <int NX, int NY, int NZ, bool IN8, bool OUT8>
__global__ void __launch_bounds__(BLOCK_THREADS) block_roundtrip_topn_kernel(const BlockRtTopnArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	block_load_x<NX, NY, NZ, KIND_REDFT10, IN8>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in, a.in8, lds, bin, cnt, tid);
	__syncthreads();
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, NZ == 1), lds, cnt, tid); __syncthreads(); }
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 2, true), lds, cnt, tid); __syncthreads(); }
	// a wave owns a block (blocks of 16 or 32 elements: 4 or 2 to a wave).  The lane that holds element 0 keeps the block's DC as it was
	// before the selection (motion.c:650) and puts it back where the filter's preserve_dc = dc would read it (:734).
	{
		constexpr int E = NX * NY * NZ, L = E >= 64 ? 64 : E, K = E >= 64 ? E / 64 : 1, PER_WAVE = 64 / L;
		static_assert(K * L == E && (L & (L - 1)) == 0, "block sizes are 16, 32 or a multiple of 64 elements");
		const bool restore = motion_filter_restores_dc(a.filt);
		const int sub = (tid & 63) / L, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
		for (int g0 = wave * PER_WAVE; g0 < cnt; g0 += (BLOCK_THREADS / 64) * PER_WAVE) {
			const int g = g0 + sub;
			const bool active = g < cnt, lead = active && (tid & (L - 1)) == 0;
			float *blk = lds + (active ? g : g0) * NX;
			float dc = 0.f;
			if (restore && lead) dc = blk[0];
			topn_select_lds<K, NX>(blk, a.pitch, E, a.keep, L, active);
			if (restore && lead) blk[0] = dc;
		}
	}
	__syncthreads();
	unsigned long long mine = 0;
	if (a.filt.enabled) {
		const int cols = cnt * NX;
		for (int l = tid; l < NZ * NY * cols; l += BLOCK_THREADS) {
			const int row = l / cols, c = l - row * cols;
			const int bz = row / NY, by = row - bz * NY, bx = c % NX;
			if (bx < a.filt.aw && by < a.filt.ah && bz < a.filt.ad) {
				float *p = lds + row * a.pitch + c;
				*p = motion_filter_at(a.filt, bz, by, bx, *p, mine);
			}
		}
		__syncthreads();
	}
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 2, false), lds, cnt, tid); __syncthreads(); }
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, cnt, tid); __syncthreads(); }
	if (a.filt.enabled && a.coded) {
		unsigned int m = (unsigned int)mine;
		for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
		if ((tid & 63) == 0 && m) atomicAdd(&wg_coded, m);
		__syncthreads();
		if (tid == 0 && wg_coded) atomicAdd(a.coded, (unsigned long long)wg_coded);
	}
	// the inverse's global scale rides on its x pass, the last one here
	block_store_x<NX, NY, NZ, KIND_REDFT01, OUT8>(a, block_axis_args(a.i, 0, true), a.out, a.out8, a.mul8, lds, bout, cnt, tid);
}

template <int NX, int NY, int NZ, bool IN8, bool OUT8>
static int launch_block_rt_topn(const BlockRtTopnArgs &a, int nwg, size_t lds, void *stream)
{
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_roundtrip_topn_kernel<NX, NY, NZ, IN8, OUT8>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL((block_roundtrip_topn_kernel<NX, NY, NZ, IN8, OUT8>), dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
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
