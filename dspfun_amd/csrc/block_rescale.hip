// block_rescale.hip -- motion -b with -s over a block grid (motion --blocksize 8x8x8 --size 4x4x4 and the like): the fused small-block
// roundtrip whose inverse runs over other extents than its forward transform, every block of the grid in ONE launch.  The phases are
// block_rs_core.h's; one kernel serves every pair of extents and every kind of end (float, 8-bit, 8-bit with motion --linear's tables),
// each phase chosen by a switch that is uniform over the workgroup.  The table staging and the coded-count reduction are block_rt.h's.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rs_core.h"
#include "block_rt.h"

namespace dspfft {

// dynamic LDS: the tile | the transfer characteristic's tables (TrcU8Tab's layout) | the workgroup's coded count
__global__ void __launch_bounds__(BLOCK_THREADS) block_rescale_kernel(const BlockRsArgs args)
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
	// (an end that is not 8-bit has no table)
	const BlockTrc t = block_trc_stage(a.in8 ? args.tab_in : nullptr, a.out8 ? args.tab_out : nullptr, args.trc_out, behind, tid);
	rs_phase_load(a, lds, bin, cnt, tid, t.lut);
	__syncthreads();
	if (a.nz > 1) { rs_phase_fwd_y(a, lds, cnt, tid); __syncthreads(); }
	unsigned long long mine = 0;
	rs_phase_mid(a, lds, cnt, tid, mine);
	__syncthreads();
	if (a.nz > 1) { rs_phase_inv_y(a, lds, cnt, tid); __syncthreads(); }
	if (a.filt.enabled && args.coded) block_coded_add(mine, wg_coded, args.coded);
	rs_phase_store(a, lds, bout, cnt, tid, t.thr, args.trc_out);
}

}  // namespace dspfft

/* rt_run_grid's launch (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without this unit).  lds: the
 * tile's bytes; the tables and the counter follow it.  -1: extents without a kernel, or a tile that does not fit. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_rescale_launch(const dspfft::BlockRsArgs *ap, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockRsArgs &a = *ap;
	const bool two_d = a.nz == 1 && a.oz == 1;
	if (!rs_extent_ok(a.nx, two_d) || !rs_extent_ok(a.ox, two_d) || !rs_extent_ok(a.ny, two_d) || !rs_extent_ok(a.oy, two_d) ||
	    !(two_d || (rs_extent_ok(a.nz, false) && rs_extent_ok(a.oz, false)))) return -1;
	if (lds != rs_tile_bytes(rs_tile_of(a)) || (lds & 15) || a.G < 1 || a.pitch != a.G * a.tw || a.tw != rs_max(a.nx, a.ox) || nwg < 1) return -1;
	lds += sizeof(TrcU8Tab) + 16;
	if (lds > 64 * 1024) return -1;
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_rescale_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	hipLaunchKernelGGL(block_rescale_kernel, dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}
