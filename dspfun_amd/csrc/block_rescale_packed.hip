// block_rescale_packed.hip -- motion -b with -s over a block grid on packed 8-bit pixels (rgb24, rgba ...: dspfft_execute_roundtrip_u8_packed_rescale):
// block_rescale.hip's one launch with block_rs_packed_core.h's packed ends and per-component mid phase.  One kernel per number of components
// serves every pair of extents and both kinds of end (plain, motion --linear's tables), each phase chosen by a switch that is uniform over the
// workgroup.  The table staging and the coded-count reduction are block_rt.h's.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rs_packed_core.h"
#include "block_rt.h"

namespace dspfft {

// dynamic LDS: the tile | the transfer characteristic's tables (TrcU8Tab's layout) | the workgroup's coded count
template <int C>
__global__ void __launch_bounds__(BLOCK_THREADS) block_rescale_packed_kernel(const BlockRsPackedArgs args)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	float *lds = reinterpret_cast<float *>(lds_raw);
	const RsTile a = rs_tile_of(args);
	unsigned char *behind = lds_raw + rs_tile_bytes(a);
	unsigned int *wg_coded = reinterpret_cast<unsigned int *>(behind + sizeof(TrcU8Tab));
	const int tid = threadIdx.x;
	if (tid == 0) *wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(args, blockIdx.x, bin, bout, cnt);
	const BlockTrc t = block_trc_stage(args.tab_in, args.tab_out, args.trc_out, behind, tid);
	rs_packed_phase_load<C>(a, lds, bin, cnt, tid, t.lut);
	__syncthreads();
	const int nb = cnt * C;           // the tile's blocks
	if (a.nz > 1) { rs_phase_fwd_y(a, lds, nb, tid); __syncthreads(); }
	unsigned long long mine = 0;
	rs_packed_phase_mid<C>(a, args, lds, cnt, tid, mine);
	__syncthreads();
	if (a.nz > 1) { rs_phase_inv_y(a, lds, nb, tid); __syncthreads(); }
	if (a.filt.enabled && args.coded) block_coded_add(mine, wg_coded, args.coded);
	rs_packed_phase_store<C>(a, lds, bout, cnt, tid, t.thr, t.tp);
}

template <int C>
static int launch_block_rescale_packed(const BlockRsPackedArgs &a, int nwg, size_t lds, void *stream)
{
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_rescale_packed_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL(block_rescale_packed_kernel<C>, dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}

}  // namespace dspfft

/* rt_run_packed_grid's launch (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without this unit).  lds: the
 * tile's bytes; the tables and the counter follow it.  -1: extents or a number of components without a kernel, or a tile that does not fit. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_rescale_packed_launch(const dspfft::BlockRsPackedArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockRsPackedArgs &a = *ap;
	const bool two_d = a.nz == 1 && a.oz == 1;
	if (!rs_extent_ok(a.nx, two_d) || !rs_extent_ok(a.ox, two_d) || !rs_extent_ok(a.ny, two_d) || !rs_extent_ok(a.oy, two_d) ||
	    !(two_d || (rs_extent_ok(a.nz, false) && rs_extent_ok(a.oz, false)))) return -1;
	if (!a.in8 || !a.out8 || a.comps < 2 || a.comps > PACKED_MAX_COMPS) return -1;
	if (lds != rs_tile_bytes(rs_tile_of(a)) || (lds & 15) || a.G < 1 || a.pitch != a.comps * a.G * a.tw || a.tw != rs_min(a.nx, a.ox) || nwg < 1) return -1;
	lds += sizeof(TrcU8Tab) + 16;
	if (lds > 64 * 1024) return -1;
	switch (a.comps) {
	case 2: return launch_block_rescale_packed<2>(a, nwg, lds, stream);
	case 3: return launch_block_rescale_packed<3>(a, nwg, lds, stream);
	case 4: return launch_block_rescale_packed<4>(a, nwg, lds, stream);
	}
	return -1;
}
