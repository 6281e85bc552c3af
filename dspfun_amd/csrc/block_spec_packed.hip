// block_spec_packed.hip -- motion --spectrogram and --ispectrogram over small blocks of packed 8-bit pixels (rgb24, rgba ...:
// dspfft_execute_spectrogram_u8_packed / _ispectrogram_u8_packed), each ONE launch: block_spec.hip's two sequences of phases with
// block_packed_core.h's linear ends and block_spec_packed_core.h's encoded ends, over DSPFFT_BLOCK_SHAPES x C in {2, 3, 4}, and their dispatch.
#include <hip/hip_runtime.h>
#include "backend.h"
#include "block_rt.h"
#include "block_spec_packed_core.h"

namespace dspfft {

// packed load, REDFT10 along x, y, z | every component block's DC from the tile, its filter, encode, packed store
// RF (both kernels): the launch's rows_fast as a constant.  block_line_of's two orders of (row, block) behind a run-time switch left the pair
// in scratch memory for some extents (4-point lines with 16 rows or planes); with the order known at compile time it stays in registers.
template <int NX, int NY, int NZ, int C, bool RF>
__global__ void __launch_bounds__(BLOCK_THREADS) block_spec_packed_kernel(const BlockSpecPackedArgs arg)
{
	BlockSpecPackedArgs a = arg;
	a.rows_fast = RF;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(arg, blockIdx.x, bin, bout, cnt);
	packed_load_x<NX, NY, NZ, C>(a, block_axis_args(a.f, 0, NY == 1 && NZ == 1), a.in8, lds, bin, cnt, tid, nullptr);
	__syncthreads();
	const int nb = cnt * C;           // the tile's blocks
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 1, NZ == 1), lds, nb, tid); __syncthreads(); }
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT10>(a, block_axis_args(a.f, 2, true), lds, nb, tid); __syncthreads(); }
	unsigned long long mine = 0;
	packed_spec_store<NX, NY, NZ, C>(a, lds, bout, cnt, tid, mine);
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
}

// packed load, decode, the component's filter | REDFT01 along z, y, x, quantised packed store
template <int NX, int NY, int NZ, int C, bool RF>
__global__ void __launch_bounds__(BLOCK_THREADS) block_ispec_packed_kernel(const BlockSpecPackedArgs arg)
{
	BlockSpecPackedArgs a = arg;
	a.rows_fast = RF;
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	__shared__ unsigned int wg_coded;
	float *lds = reinterpret_cast<float *>(lds_raw);
	const int tid = threadIdx.x;
	if (tid == 0) wg_coded = 0;
	long long bin, bout;
	int cnt;
	block_base(arg, blockIdx.x, bin, bout, cnt);
	unsigned long long mine = 0;
	packed_ispec_load<NX, NY, NZ, C>(a, lds, bin, cnt, tid, mine);
	__syncthreads();
	const int nb = cnt * C;
	if constexpr (NZ > 1) { block_lines_z<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 2, false), lds, nb, tid); __syncthreads(); }
	if constexpr (NY > 1) { block_lines_y<NX, NY, NZ, KIND_REDFT01>(a, block_axis_args(a.i, 1, false), lds, nb, tid); __syncthreads(); }
	if (a.filt.enabled && a.coded) block_coded_add(mine, &wg_coded, a.coded);
	// the plan's global scale rides on the x pass, the last one here
	packed_store_x<NX, NY, NZ, C>(a, block_axis_args(a.i, 0, true), a.out8, a.mul8, lds, bout, cnt, tid, nullptr, TrcParams());
}

template <int NX, int NY, int NZ, int C, bool RF>
static int launch_block_spec_packed_rf(const BlockSpecPackedArgs &a, int inverse, int nwg, size_t lds, void *stream)
{
	static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_spec_packed_kernel<NX, NY, NZ, C, RF>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) |
	                  (int)hipFuncSetAttribute(reinterpret_cast<const void *>(block_ispec_packed_kernel<NX, NY, NZ, C, RF>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
	if (attr) return attr;
	if (inverse) hipLaunchKernelGGL((block_ispec_packed_kernel<NX, NY, NZ, C, RF>), dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	else hipLaunchKernelGGL((block_spec_packed_kernel<NX, NY, NZ, C, RF>), dim3(nwg), dim3(BLOCK_THREADS), lds, (hipStream_t)stream, a);
	return (int)hipGetLastError();
}
template <int NX, int NY, int NZ, int C>
static int launch_block_spec_packed(const BlockSpecPackedArgs &a, int inverse, int nwg, size_t lds, void *stream)
{
	return a.rows_fast ? launch_block_spec_packed_rf<NX, NY, NZ, C, true>(a, inverse, nwg, lds, stream) : launch_block_spec_packed_rf<NX, NY, NZ, C, false>(a, inverse, nwg, lds, stream);
}

template <int NX, int NY, int NZ>
static int launch_block_spec_packed_c(const BlockSpecPackedArgs &a, int inverse, int nwg, size_t lds, void *stream)
{
	switch (a.comps) {
	case 2: return launch_block_spec_packed<NX, NY, NZ, 2>(a, inverse, nwg, lds, stream);
	case 3: return launch_block_spec_packed<NX, NY, NZ, 3>(a, inverse, nwg, lds, stream);
	case 4: return launch_block_spec_packed<NX, NY, NZ, 4>(a, inverse, nwg, lds, stream);
	}
	return -1;
}

}  // namespace dspfft

/* spec_packed_block's launch (engine.cpp reaches this through a weak reference: the CPU emulation links engine.cpp without this unit).  lds:
 * the tile's bytes.  -1: no kernel for these block extents or this number of components, or a tile that does not fit or does not match the
 * geometry. */
extern "C" __attribute__((visibility("hidden"))) int dspfft_block_spec_packed_launch(const dspfft::BlockSpecPackedArgs *ap, int inverse, int nwg, size_t lds, void *stream)
{
	using namespace dspfft;
	const BlockSpecPackedArgs &a = *ap;
	if (!a.in8 || !a.out8 || nwg < 1 || a.G < 1 || a.pitch != a.G * a.comps * a.nx || lds != (size_t)a.nz * a.ny * a.pitch * sizeof(float) || lds + 16 > 64 * 1024) return -1;
#define DSP_BLOCK_CASE(X_, Y_, Z_) \
	if (a.nx == X_ && a.ny == Y_ && a.nz == Z_) return launch_block_spec_packed_c<X_, Y_, Z_>(a, inverse, nwg, lds, stream);
	DSPFFT_BLOCK_SHAPES(DSP_BLOCK_CASE)
#undef DSP_BLOCK_CASE
	return -1;
}
