// temporal_rt.hip -- motion -b 1x1xD (-s 1x1xD'): the fused roundtrip over blocks that exist only along time, every block and every pixel
// column of a [frames][H][W] plane in ONE launch.  The phases are temporal_core.h's; one kernel serves every pair of lengths and every kind
// of end (float, 8-bit, 8-bit with motion --linear's tables), each chosen by a switch that is uniform over the workgroup.  The table staging
// and the coded-count reduction are block_rt.h's.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "temporal_core.h"
#include "block_rt.h"

namespace dspfft {

// dynamic LDS: the tile | the transfer characteristic's tables (TrcU8Tab's layout) | the workgroup's coded count
template <int NT>
__global__ void __launch_bounds__(NT) temporal_rt_kernel(const TemporalArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	cx<float> *buf = reinterpret_cast<cx<float> *>(lds_raw);
	unsigned char *behind = lds_raw + temporal_tile_bytes(a);
	unsigned int *wg_coded = reinterpret_cast<unsigned int *>(behind + sizeof(TrcU8Tab));
	const int tid = threadIdx.x;
	if (tid == 0) *wg_coded = 0;
	long long bin, bout;
	int valid;
	temporal_base(a, blockIdx.x, bin, bout, valid);
	// (an end that is not 8-bit has no table)
	const BlockTrc t = block_trc_stage(a.in8 ? a.tab_in : nullptr, a.out8 ? a.tab_out : nullptr, a.trc_out, behind, tid);
	temporal_phase_load(a, buf, bin, valid, tid, NT, t.lut);
	__syncthreads();
	for (int s = 0; s < a.ff.ns; s++) { temporal_stage(a, buf, false, s, tid, NT); __syncthreads(); }
	unsigned long long mine = 0;
	{
		TemporalHeld h;
		temporal_post_read(a, buf, valid, tid, NT, h);
		__syncthreads();
		temporal_post_write(a, buf, valid, tid, NT, h, mine);
	}
	__syncthreads();
	temporal_pre(a, buf, valid, tid, NT);
	__syncthreads();
	for (int s = 0; s < a.fi.ns; s++) { temporal_stage(a, buf, true, s, tid, NT); __syncthreads(); }
	if (a.filt.enabled && a.coded) block_coded_add(mine, wg_coded, a.coded);
	temporal_phase_store(a, buf, bout, valid, tid, NT, t.thr, a.trc_out);
}

template <int NT>
static int temporal_launch(const TemporalArgs &a, int nwg, size_t lds, hipStream_t stream)
{
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(temporal_rt_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
	                                           TEMPORAL_TILE_BYTES + sizeof(TrcU8Tab) + 16);
	if (attr) return attr;
	hipLaunchKernelGGL(temporal_rt_kernel<NT>, dim3(nwg), dim3(NT), lds, stream, a);
	return (int)hipGetLastError();
}

}  // namespace dspfft

/* rt_run_temporal's launch (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without this unit).  The
 * geometry is checked once more, against what the kernel's index arithmetic and its held registers rely on.  -1: a geometry it cannot run. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_temporal_rt_launch(const dspfft::TemporalArgs *ap, int nwg, void *stream)
{
	using namespace dspfft;
	const TemporalArgs &a = *ap;
	const int m = a.D > a.S ? a.D : a.S;
	if (a.D < 2 || a.S < 2 || a.K < 4 || (a.K & 3) || a.B * 2 != a.K || a.P < 4 || (a.P & 3) || a.ntiles != (a.P + a.K - 1) / a.K || nwg < 1) return -1;
	if (a.ff.L != a.D || a.fi.L != a.S || a.ff.ns < 1 || a.fi.ns < 1 || a.ff.ns > 8 || a.fi.ns > 8) return -1;
	if (a.divB.d != (uint32_t)a.B || a.divQ.d != (uint32_t)(a.K / 4) || a.div_tiles.d != (uint32_t)a.ntiles) return -1;
	const size_t tile = temporal_tile_bytes(a);
	if (tile > TEMPORAL_TILE_BYTES) return -1;
	const int nthr = temporal_threads(m, a.K);
	if ((long long)(a.D / 2 + 1) * a.B > (long long)TEMPORAL_HOLD * nthr) return -1;
	const size_t lds = tile + sizeof(TrcU8Tab) + 16;
	return nthr == 512 ? temporal_launch<512>(a, nwg, lds, (hipStream_t)stream) : temporal_launch<256>(a, nwg, lds, (hipStream_t)stream);
}
