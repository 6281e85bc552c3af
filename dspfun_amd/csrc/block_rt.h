// block_rt.h -- the fused small-block roundtrip's kernels, each sequence of block_core.h phases stated once: the plain one
// (block_roundtrip_kernel) and the one with motion --coeff-limit's selection before the filter (block_roundtrip_topn_kernel).  Both are
// templates on their argument structure; with BlockRtTrcArgs they put motion --linear's tables at the 8-bit ends, in LDS behind the tile.
// block_fused.hip, block_topn.hip and block_trc.hip instantiate and dispatch them, one argument structure each; block_rescale.hip shares the
// table staging and the coded-count reduction.  engine.cpp and the CPU emulation see the argument structure only.
#pragma once
#include <type_traits>
#include "block_core.h"
#include "topn_core.h"

namespace dspfft {

// the roundtrip's arguments plus the 8-bit ends' tables (a plan's device tables; NULL: that end converts plainly)
struct BlockRtTrcArgs : BlockRtTopnArgs {
	const TrcU8Tab *tab_in, *tab_out;
	int trc_out;                  // the id behind tab_out (its parameters seed the threshold search)
};

#if defined(__HIP__)
// copy the tables of the ends that have one (NULL: that end converts plainly) into LDS at `at` (16-byte aligned, TrcU8Tab's layout); the
// caller's first barrier covers the copy
__device__ __forceinline__ BlockTrc block_trc_stage(const TrcU8Tab *tab_in, const TrcU8Tab *tab_out, int trc_out, unsigned char *at, int tid)
{
	BlockTrc t = {nullptr, nullptr, TrcParams()};
	double *thr = reinterpret_cast<double *>(at);
	float *lut = reinterpret_cast<float *>(at + sizeof(double) * 256);
	if (tab_out) { for (int i = tid; i < 256; i += BLOCK_THREADS) thr[i] = tab_out->thr[i]; t.thr = thr; t.tp = trc_params(trc_out); }
	if (tab_in) {
		for (int i = tid; i < 256; i += BLOCK_THREADS) lut[i] = tab_in->lut[i];
		t.lut = lut;
		__syncthreads();          // the load below reads the table
	}
	return t;
}

// the coefficients the workgroup's lanes counted as coded (`mine` each) into the global counter: a shuffle tree per wave, the waves through
// *wg_coded in LDS (zeroed before an earlier barrier).  Every thread of the workgroup calls this or none does: it holds a barrier.
__device__ __forceinline__ void block_coded_add(unsigned long long mine, unsigned int *wg_coded, unsigned long long *coded)
{
	unsigned int m = (unsigned int)mine;
	for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(wg_coded, m);
	__syncthreads();
	if (threadIdx.x == 0 && *wg_coded) atomicAdd(coded, (unsigned long long)*wg_coded);
}

// The sequences are kernel templates, not functions that each unit's kernel calls: called as functions the compiler built other code for
// them than it builds for a kernel (a branchy filter sweep in the top-N sequence, 2.5 % on 8x8x8 blocks; profiles/r10_block_roundtrip_owner.txt).
// motion's per-block pipeline in one pass: load (float / 8-bit), REDFT10 along x, y, z, filter, REDFT01 along z, y, x, store
template <int NX, int NY, int NZ, bool IN8, bool OUT8, class Args>
__global__ void __launch_bounds__(BLOCK_THREADS) block_roundtrip_kernel(const Args a)
{
	constexpr bool TRC = std::is_same<Args, BlockRtTrcArgs>::value;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	BlockTrc tabs;
	const BlockTrc *t = nullptr;
	if constexpr (TRC) { tabs = block_trc_stage(a.tab_in, a.tab_out, a.trc_out, lds_raw + (size_t)NZ * NY * a.pitch * sizeof(float), tid); t = &tabs; }
	block_load_x<NX, NY, NZ, KIND_REDFT10, IN8, TRC>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in, a.in8, lds, bin, cnt, tid, t);
	__syncthreads();
	// the last forward axis, the filter and the same axis of the inverse run on one line in registers (block_lines_mid)
	unsigned long long mine = 0;
	if constexpr (NZ > 1) {
		if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, false), lds, cnt, tid); __syncthreads(); }
		block_lines_mid<NX, NY, NZ, true>(a, block_axis_args(a.f, 2, true), block_axis_args(a.i, 2, false), a.filt, lds, cnt, tid, mine);
		__syncthreads();
		if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, cnt, tid); __syncthreads(); }
	} else {
		block_lines_mid<NX, NY, NZ, false>(a, block_axis_args(a.f, 1, true), block_axis_args(a.i, 1, false), a.filt, lds, cnt, tid, mine);
		__syncthreads();
	}
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
	// the inverse's global scale rides on its x pass, the last one here
	block_store_x<NX, NY, NZ, KIND_REDFT01, OUT8, TRC>(a, block_axis_args(a.i, 0, true), a.out, a.out8, a.mul8, lds, bout, cnt, tid, t);
}

// load (float / 8-bit), REDFT10 along x, y, z | per-block top-N (topn_core.h, motion.c:652-668) | filter | REDFT01 along z, y, x, store: the
// middle is unfused, because the selection needs the whole block's coefficients before any of them is filtered
template <int NX, int NY, int NZ, bool IN8, bool OUT8, class Args>
__global__ void __launch_bounds__(BLOCK_THREADS) block_roundtrip_topn_kernel(const Args a)
{
	constexpr bool TRC = std::is_same<Args, BlockRtTrcArgs>::value;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	BlockTrc tabs;
	const BlockTrc *t = nullptr;
	if constexpr (TRC) { tabs = block_trc_stage(a.tab_in, a.tab_out, a.trc_out, lds_raw + (size_t)NZ * NY * a.pitch * sizeof(float), tid); t = &tabs; }
	block_load_x<NX, NY, NZ, KIND_REDFT10, IN8, TRC>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in, a.in8, lds, bin, cnt, tid, t);
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
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
	// the inverse's global scale rides on its x pass, the last one here
	block_store_x<NX, NY, NZ, KIND_REDFT01, OUT8, TRC>(a, block_axis_args(a.i, 0, true), a.out, a.out8, a.mul8, lds, bout, cnt, tid, t);
}

#endif

}  // namespace dspfft
