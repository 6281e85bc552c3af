// topn_core.h -- motion --coeff-limit per block (motion/motion.c:652-668): keep the `keep` coefficients of largest magnitude of ONE block
// that lies in LDS, zero the rest, in place.  Shared by the fused block kernel (block_topn.hip: the blocks of a tile [NZ][NY][G * NX]) and by
// the batched stand-alone call (motion_ops.hip: contiguous runs), so that both apply the same rule with the same code:
//   key     the bit pattern of |c| (monotone for non-negative floats); NaNs are outside the contract (the reference's qsort comparator is
//           undefined on them and motion's inputs cannot produce them)
//   ties    at the threshold the earliest in the block's own buffer order (z, then y, then x) are kept; the reference leaves them to qsort
// The reference selects over `mincomponent`, the largest component's buffer: for a smaller component the remainder is zeros, so per block
// the selection runs over the block's own embedding, which is what the callers hand in here.
// How: a group of L lanes (a whole wave for blocks of 64 elements and more; 64 / L blocks share a wave below that) holds the block's keys in
// registers, K = ceil(E / L) per lane, element e in lane e % L, chunk e / L.  The threshold T -- the keep-th largest key -- is found bit by bit
// from the top: 31 rounds of compare + __ballot + popcount, no atomics, no LDS beside the block itself.  Keys above T stay, and of the keys
// equal to T the first keep - #{key > T}, ranked by ballot prefix within a chunk plus a running count over the chunks.
#pragma once
#include "block_core.h"

namespace dspfft {

// BlockRtArgs plus the coefficient limit (block_topn.hip's kernel; the plain kernel's arguments stay as they are)
struct BlockRtTopnArgs : BlockRtArgs {
	unsigned int keep;            // 0 < keep < nx * ny * nz
};

// motion.c:730-735: does the filter put the block's DC back (preserve_dc = dc)?  Then it is the value from BEFORE the selection (:650).
DSP_HD bool motion_filter_restores_dc(const MotionFilter &p)
{
	return p.enabled && p.preserve_dc == 1 && (p.b0d || p.b0h || p.b0w || p.boost != 1.f || p.thr_hi > 0.f);
}

#if defined(__HIP__)         // (engine.cpp and the CPU emulation see the declarations above only)
// All 64 lanes of the wave call this together (the ballots need them); a lane group without a block passes active = false.
// K: keys per lane (K * L >= E).  L: lanes per block, 64 or a smaller power of two; the group of lane w is lanes [w & ~(L - 1), +L).
// NX: the block's rows are NX elements long and `pitch` floats apart (L a multiple of NX, or K = 1); NX = 0: one contiguous run.
template <int K, int NX>
__device__ inline __attribute__((always_inline)) void topn_select_lds(float *blk, int pitch, int E, unsigned int keep, int L, bool active)
{
	const int w = (int)(threadIdx.x & 63u), sl = w & (L - 1);
	const unsigned long long gm = L >= 64 ? ~0ull : (((1ull << L) - 1ull) << (w - sl));   // my group's lanes
	const unsigned long long before = gm & ((1ull << w) - 1ull);                         // ... those ahead of me
	// element e = j L + sl (chunk j) lies at first + j step
	int first = NX ? (sl / (NX ? NX : 1)) * pitch + sl % (NX ? NX : 1) : sl;
	const int step = NX ? (L / (NX ? NX : 1)) * pitch : L;
	uint32_t key[K];
#pragma unroll
	for (int j = 0; j < K; j++)
		key[j] = (active && j * L + sl < E) ? (__float_as_uint(blk[first + j * step]) & 0x7fffffffu) : 0u;   // (an absent element never reaches a threshold >= 1)
	DSP_PIN1(first);                      // the stores below form their addresses again instead of keeping K of them in registers through the rounds
	uint32_t T = 0;
#pragma unroll 1
	for (int b = 30; b >= 0; b--) {
		const uint32_t cand = T | (1u << b);
		uint32_t cnt = 0;
#pragma unroll
		for (int j = 0; j < K; j++) {
			cnt += (uint32_t)__popcll(__ballot(key[j] >= cand) & gm);
			if ((j & 7) == 7) DSP_SCHED_FENCE();      // (eight compares in flight, not K: their masks are scalar register pairs)
		}
		if (cnt >= keep) T = cand;
	}
	uint32_t above = 0;
#pragma unroll
	for (int j = 0; j < K; j++) {
		above += (uint32_t)__popcll(__ballot(key[j] > T) & gm);
		if ((j & 7) == 7) DSP_SCHED_FENCE();
	}
	const uint32_t ties = keep - above;         // >= 1: fewer than `keep` keys lie above the keep-th largest
	uint32_t seen = 0;
#pragma unroll
	for (int j = 0; j < K; j++) {
		const bool tie = key[j] == T;
		const unsigned long long m = __ballot(tie) & gm;
		const bool kept = key[j] > T || (tie && seen + (uint32_t)__popcll(m & before) < ties);
		if (active && j * L + sl < E && !kept) blk[first + j * step] = 0.f;
		seen += (uint32_t)__popcll(m);
		if ((j & 3) == 3) DSP_SCHED_FENCE();
	}
}
#endif

}  // namespace dspfft
