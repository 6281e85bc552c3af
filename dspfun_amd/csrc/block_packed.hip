// block_packed.hip -- the fused small-block roundtrip on packed 8-bit pixels (rgb24, rgba ...: dspfft_execute_roundtrip_u8_packed): block_rt.h's two
// sequences of phases, the plain one and the one with motion --coeff-limit's selection, with block_packed_core.h's ends and per-component filter,
// over DSPFFT_BLOCK_SHAPES x C in {2, 3, 4}, and their dispatch.  One argument structure: the tables of motion --linear are staged in LDS behind the
// tile when the call has any (a NULL pointer: that end converts plainly).
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rt.h"
#include "block_packed_core.h"

namespace dspfft {

// load, REDFT10 along x, y, z, filter, REDFT01 along z, y, x, store (block_roundtrip_kernel's sequence)
template <int NX, int NY, int NZ, int C>
__global__ void __launch_bounds__(BLOCK_THREADS) block_packed_kernel(const BlockPackedArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	const BlockTrc t = block_trc_stage(a.tab_in, a.tab_out, a.trc_out, lds_raw + (size_t)NZ * NY * a.pitch * sizeof(float), tid);
	packed_load_x<NX, NY, NZ, C>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in8, lds, bin, cnt, tid, t.lut);
	__syncthreads();
	const int nb = cnt * C;           // the tile's blocks
	unsigned long long mine = 0;
	if constexpr (NZ > 1) {
		if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, false), lds, nb, tid); __syncthreads(); }
		packed_lines_mid<NX, NY, NZ, C, true>(a, block_axis_args(a.f, 2, true), block_axis_args(a.i, 2, false), lds, cnt, tid, mine);
		__syncthreads();
		if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, nb, tid); __syncthreads(); }
	} else {
		packed_lines_mid<NX, NY, NZ, C, false>(a, block_axis_args(a.f, 1, true), block_axis_args(a.i, 1, false), lds, cnt, tid, mine);
		__syncthreads();
	}
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
	// the inverse's global scale rides on its x pass, the last one here
	packed_store_x<NX, NY, NZ, C>(a, block_axis_args(a.i, 0, true), a.out8, a.mul8, lds, bout, cnt, tid, t.thr, t.tp);
}

// load, REDFT10 along x, y, z | per-block top-N | filter | REDFT01 along z, y, x, store (block_roundtrip_topn_kernel's sequence): every
// component block selects for itself (motion.c:652-668 runs inside the loop over components, :613-615)
template <int NX, int NY, int NZ, int C>
__global__ void __launch_bounds__(BLOCK_THREADS) block_packed_topn_kernel(const BlockPackedArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	const BlockTrc t = block_trc_stage(a.tab_in, a.tab_out, a.trc_out, lds_raw + (size_t)NZ * NY * a.pitch * sizeof(float), tid);
	packed_load_x<NX, NY, NZ, C>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in8, lds, bin, cnt, tid, t.lut);
	__syncthreads();
	const int nb = cnt * C;
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, NZ == 1), lds, nb, tid); __syncthreads(); }
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 2, true), lds, nb, tid); __syncthreads(); }
	// a wave owns a block (blocks of 16 or 32 elements: 4 or 2 to a wave); the lane that holds element 0 keeps the block's DC as it was before
	// the selection (motion.c:650) for the components whose filter restores it (:734)
	{
		constexpr int E = NX * NY * NZ, L = E >= 64 ? 64 : E, K = E >= 64 ? E / 64 : 1, PER_WAVE = 64 / L;
		static_assert(K * L == E && (L & (L - 1)) == 0, "block sizes are 16, 32 or a multiple of 64 elements");
		const int sub = (tid & 63) / L, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
		for (int g0 = wave * PER_WAVE; g0 < nb; g0 += (BLOCK_THREADS / 64) * PER_WAVE) {
			const int g = g0 + sub;
			const bool active = g < nb, lead = active && (tid & (L - 1)) == 0;
			const bool restore = motion_filter_restores_dc(packed_filter_of<C>(a, packed_comp_of<C>(active ? g : g0, cnt)));
			float *blk = lds + (active ? g : g0) * NX;
			float dc = 0.f;
			if (restore && lead) dc = blk[0];
			topn_select_lds<K, NX>(blk, a.pitch, E, a.keep, L, active);
			if (restore && lead) blk[0] = dc;
		}
	}
	__syncthreads();
	unsigned long long mine = 0;
	if (a.filt.enabled) { packed_filter_sweep<NX, NY, NZ, C>(a, lds, cnt, tid, mine); __syncthreads(); }
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 2, false), lds, nb, tid); __syncthreads(); }
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, nb, tid); __syncthreads(); }
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
	packed_store_x<NX, NY, NZ, C>(a, block_axis_args(a.i, 0, true), a.out8, a.mul8, lds, bout, cnt, tid, t.thr, t.tp);
}

template <int NX, int NY, int NZ, int C, bool TOPN>
static int launch_block_packed(const BlockPackedArgs &a, int nwg, size_t lds, void *stream)
{
	const auto kern = TOPN ? &block_packed_topn_kernel<NX, NY, NZ, C> : &block_packed_kernel<NX, NY, NZ, C>;
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
