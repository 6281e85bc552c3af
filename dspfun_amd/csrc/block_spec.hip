// block_spec.hip -- motion --spectrogram and --ispectrogram over small blocks, each ONE launch: the halves of the fused block roundtrip
// (block_rt.h) with block_spec_core.h's encode and decode phases at the cut.  Pixels are 8-bit or float at both ends of a call; the mode is a
// switch that is uniform over the launch.  The coded-count reduction is block_rt.h's.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_spec_core.h"
#include "block_rt.h"

namespace dspfft {

// load (8-bit / float), REDFT10 along x, y, z | the block's DC from the tile, filter, encode, store
template <int NX, int NY, int NZ, bool U8>
__global__ void __launch_bounds__(BLOCK_THREADS) block_spec_kernel(const BlockSpecArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	block_load_x<NX, NY, NZ, KIND_REDFT10, U8>(a, block_axis_args(a.s, 0, NY == 1 && NZ == 1), a.in, a.in8, lds, bin, cnt, tid);
	__syncthreads();
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.s, 1, NZ == 1), lds, cnt, tid); __syncthreads(); }
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.s, 2, true), lds, cnt, tid); __syncthreads(); }
	unsigned long long mine = 0;
	block_spec_store<NX, NY, NZ, U8>(a, lds, bout, cnt, tid, mine);
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
}

// load, decode, filter | REDFT01 along z, y, x, store (float / quantised 8-bit)
template <int NX, int NY, int NZ, bool U8>
__global__ void __launch_bounds__(BLOCK_THREADS) block_ispec_kernel(const BlockSpecArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(a, blockIdx.x, bin, bout, cnt);
	unsigned long long mine = 0;
	block_ispec_load<NX, NY, NZ, U8>(a, lds, bin, cnt, tid, mine);
	__syncthreads();
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.s, 2, false), lds, cnt, tid); __syncthreads(); }
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.s, 1, false), lds, cnt, tid); __syncthreads(); }
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
	// the plan's global scale rides on the x pass, the last one here
	block_store_x<NX, NY, NZ, KIND_REDFT01, U8>(a, block_axis_args(a.s, 0, true), a.out, a.out8, a.mul8, lds, bout, cnt, tid);
}

template <int NX, int NY, int NZ, bool U8>
static int launch_block_spec(const BlockSpecArgs &a, int inverse, int nwg, size_t lds, void *stream)
{
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_spec_kernel<NX, NY, NZ, U8>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) |
	                  (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_ispec_kernel<NX, NY, NZ, U8>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	if (inverse) hipLaunchKernelGGL((block_ispec_kernel<NX, NY, NZ, U8>), dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	else hipLaunchKernelGGL((block_spec_kernel<NX, NY, NZ, U8>), dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}

}  // namespace dspfft

/* spec_block's launch (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without this unit).  a.in8 set:
 * 8-bit pixels at both ends.  -1: extents without a kernel, or a tile that does not fit. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_spec_launch(const dspfft::BlockSpecArgs *ap, int inverse, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockSpecArgs &a = *ap;
	if (nwg < 1 || a.G < 1 || a.pitch != a.G * a.nx || lds != (size_t)a.nz * a.ny * a.pitch * sizeof(float) || lds > 64 * 1024) return -1;
#define DSP_BLOCK_CASE(X_, Y_, Z_) \
	if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) \
		return a.in8 ? launch_block_spec<X_, Y_, Z_, true>(a, inverse, nwg, lds, stream) : launch_block_spec<X_, Y_, Z_, false>(a, inverse, nwg, lds, stream);
	DSPFFT_BLOCK_SHAPES(DSP_BLOCK_CASE)
#undef DSP_BLOCK_CASE
	return -1;
}
