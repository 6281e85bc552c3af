// block_packed_rt.h -- the fused small-block roundtrip's kernels on packed 8-bit pixels, each sequence of phases stated once (as block_rt.h states
// the planar ones): the plain one and the one with motion --coeff-limit's selection.  Both are templates on their argument structure:
// BlockPackedArgs ends in packed_store_x (block_packed.hip instantiates and dispatches those), BlockPackedDitherArgs in the three phases of
// motion -d (block_packed_core.h; block_packed_dither.hip).
#pragma once
#include <type_traits>
#include "block_rt.h"
#include "block_packed_core.h"

namespace dspfft {

#if defined(__HIP__)
// the dither phase's LDS: behind the tile, and behind the transfer tables when the call has any
template <int NY, int NZ, class Args>
__device__ __forceinline__ double *packed_dither_lds(const Args &a, unsigned char *lds_raw)
{
	return reinterpret_cast<double *>(lds_raw + (size_t)NZ * NY * a.pitch * sizeof(float) + ((a.tab_in || a.tab_out) ? sizeof(TrcU8Tab) : 0));
}
// its error table, staged before the sequence's first barrier (nothing to stage for the undithered call)
__device__ __forceinline__ void packed_dither_stage(const BlockPackedArgs &, double *, int) {}
__device__ __forceinline__ void packed_dither_stage(const BlockPackedDitherArgs &a, double *tab, int tid)
{
	for (int i = tid; i < 256; i += BLOCK_THREADS) tab[i] = dither_table_entry(i, a.sf, a.norm);
}
// what follows the last barrier of either sequence: the inverse's x pass (its global scale rides on it) and the store
template <int NX, int NY, int NZ, int C, class Args>
__device__ __forceinline__ void packed_store_phase(const Args &a, float *lds, unsigned char *lds_raw, long long bout, int cnt, int tid, const BlockTrc &t)
{
	if constexpr (std::is_same<Args, BlockPackedDitherArgs>::value) {
		double *tab = packed_dither_lds<NY, NZ>(a, lds_raw);
		packed_inverse_x<NX, NY, NZ, C>(a, block_axis_args(a.i, 0, true), lds, cnt, tid);
		__syncthreads();
		packed_dither_tile<NX, NY, NZ, C>(a, lds, cnt, tid, tab, tab + 256, t.thr, t.tp);
		__syncthreads();
		packed_store_bytes<NX, NY, NZ, C>(a, a.out8, lds, bout, cnt, tid);
	} else packed_store_x<NX, NY, NZ, C>(a, block_axis_args(a.i, 0, true), a.out8, a.mul8, lds, bout, cnt, tid, t.thr, t.tp);
}

// load, REDFT10 along x, y, z, filter, REDFT01 along z, y, x, store (block_roundtrip_kernel's sequence)
template <int NX, int NY, int NZ, int C, class Args>
__global__ void __launch_bounds__(BLOCK_THREADS) block_packed_kernel(const Args a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	packed_dither_stage(a, packed_dither_lds<NY, NZ>(a, lds_raw), tid);
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
	packed_store_phase<NX, NY, NZ, C>(a, lds, lds_raw, bout, cnt, tid, t);
}

// load, REDFT10 along x, y, z | per-block top-N | filter | REDFT01 along z, y, x, store (block_roundtrip_topn_kernel's sequence): every
// component block selects for itself (motion.c:652-668 runs inside the loop over components, :613-615)
template <int NX, int NY, int NZ, int C, class Args>
__global__ void __launch_bounds__(BLOCK_THREADS) block_packed_topn_kernel(const Args a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	packed_dither_stage(a, packed_dither_lds<NY, NZ>(a, lds_raw), tid);
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
	packed_store_phase<NX, NY, NZ, C>(a, lds, lds_raw, bout, cnt, tid, t);
}

#endif

}  // namespace dspfft
