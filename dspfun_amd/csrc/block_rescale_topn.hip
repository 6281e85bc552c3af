// block_rescale_topn.hip -- motion -b with -s over a block grid AND --coeff-limit (motion -b 8x8x8 -s 4x4x4 --coeff-limit 16): block_rescale.hip's
// kernel with its middle unfused, the way block_rt.h's block_roundtrip_topn_kernel unfuses block_roundtrip_kernel.  The reference ranks the
// whole max(block, scaled) embedding (motion/motion.c:652-668), so the forward passes run unpruned and leave, outside min(block, scaled), the
// values the reference ranks there (block_rs_core.h); the selection is topn_core.h's, one wave per block (or a lane group, for embeddings of
// 16 and 32 elements), on the tile itself.  Same tile, same ends, same table staging and coded count as block_rescale.hip.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rs_core.h"
#include "block_rt.h"

namespace dspfft {

// the waves take the tile's cnt blocks in turn; all 64 lanes enter the selection together (its ballots need them).  The lane that holds
// element 0 keeps the block's DC as it was before the selection (motion.c:650) and puts it back where preserve_dc = dc reads it (:734).
template <int K, int MX>
__device__ __forceinline__ void rs_select(float *lds, int tw, int pitch, int E, unsigned int keep, bool restore, int cnt, int tid)
{
	const int L = K > 1 ? 64 : E, per_wave = 64 / L;
	const int sub = (tid & 63) / L, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	for (int g0 = wave * per_wave; g0 < cnt; g0 += (BLOCK_THREADS / 64) * per_wave) {
		const int g = g0 + sub;
		const bool active = g < cnt, lead = active && (tid & (L - 1)) == 0;
		float *blk = lds + (active ? g : g0) * tw;
		float dc = 0.f;
		if (restore && lead) dc = blk[0];
		topn_select_lds<K, MX>(blk, pitch, E, keep, L, active);
		if (restore && lead) blk[0] = dc;
	}
}

// dynamic LDS: the tile | the transfer characteristic's tables (TrcU8Tab's layout) | the workgroup's coded count
__global__ void __launch_bounds__(BLOCK_THREADS) block_rescale_topn_kernel(const BlockRsTopnArgs args)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	float *lds = reinterpret_cast<float *>(lds_raw);
	const RsTile a = rs_tile_of(args), all = rs_tile_unpruned(a);
	const RsKeys keys = rs_keys_of(args);
	unsigned char *behind = lds_raw + rs_tile_bytes(a);
	unsigned int *wg_coded = reinterpret_cast<unsigned int *>(behind + sizeof(TrcU8Tab));
	const int tid = threadIdx.x;
	if (tid == 0) *wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(args, blockIdx.x, bin, bout, cnt);
	const BlockTrc t = block_trc_stage(a.in8 ? args.tab_in : nullptr, a.out8 ? args.tab_out : nullptr, args.trc_out, behind, tid);
	rs_phase_load(all, lds, bin, cnt, tid, t.lut);
	rs_phase_zero_outside(a, lds, cnt, tid);
	__syncthreads();
	if (a.nz > 1) { rs_phase_fwd_y(all, lds, cnt, tid); __syncthreads(); }
	rs_phase_fwd_last_keys(a, keys, lds, cnt, tid);
	__syncthreads();
	{
		const int E = rs_topn_elems(a);
		const bool restore = motion_filter_restores_dc(a.filt);
		switch (a.tw * 128 + rs_topn_keys(E)) {
#define DSP_RS_SEL(K_, MX_) case MX_ * 128 + K_: rs_select<K_, MX_>(lds, a.tw, a.pitch, E, args.keep, restore, cnt, tid); break;
		DSPFFT_RS_TOPN_SHAPES(DSP_RS_SEL)
#undef DSP_RS_SEL
		}
	}
	__syncthreads();
	unsigned long long mine = 0;
	rs_phase_filt_inv_last(a, lds, cnt, tid, mine);
	__syncthreads();
	if (a.nz > 1) { rs_phase_inv_y(a, lds, cnt, tid); __syncthreads(); }
	if (a.filt.enabled && args.coded) block_coded_add(mine, wg_coded, args.coded);
	rs_phase_store(a, lds, bout, cnt, tid, t.thr, args.trc_out);
}

}  // namespace dspfft

/* rt_run_grid's launch when the call carries a coefficient limit (engine.cpp reaches this through a weak reference: the CPU emulation links
 * engine.cpp without this unit).  lds: the tile's bytes; the tables and the counter follow it.  -1: extents without a kernel, a tile that does
 * not fit, or a limit that is none (0, or the whole embedding). */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_rescale_topn_launch(const dspfft::BlockRsTopnArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockRsTopnArgs &a = *ap;
	const bool two_d = a.nz == 1 && a.oz == 1;
	if (!rs_extent_ok(a.nx, two_d) || !rs_extent_ok(a.ox, two_d) || !rs_extent_ok(a.ny, two_d) || !rs_extent_ok(a.oy, two_d) ||
	    !(two_d || (rs_extent_ok(a.nz, false) && rs_extent_ok(a.oz, false)))) return -1;
	const RsTile t = rs_tile_of(a);
	if (lds != rs_tile_bytes(t) || (lds & 15) || a.G < 1 || a.pitch != a.G * a.tw || a.tw != rs_max(a.nx, a.ox) || nwg < 1) return -1;
	const int E = rs_topn_elems(t);
	bool listed = false;
#define DSP_RS_SEL(K_, MX_) listed = listed || (a.tw == MX_ && rs_topn_keys(E) == K_);
	DSPFFT_RS_TOPN_SHAPES(DSP_RS_SEL)
#undef DSP_RS_SEL
	if (!listed || a.keep < 1 || a.keep >= (unsigned int)E) return -1;
	lds += sizeof(TrcU8Tab) + 16;
	if (lds > 64 * 1024) return -1;
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_rescale_topn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL(block_rescale_topn_kernel, dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}
