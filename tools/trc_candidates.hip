// trc_candidates.hip -- the candidate evaluations of a transfer characteristic, each behind the same streaming kernel as
// dspfft_trc_apply_f32 (pointwise.hip: 16-byte accesses, grid-stride), for tools/bench_trc.py to time side by side on one device in one
// run.  Not part of the library: built by bench_trc.py into tools/libtrc_candidates.so.
//   0 copy     no arithmetic: the kernel's floor
//   1 plain    (float)trc_exact((double)x): the device library's double pow per sample
//   2 lean     trc_eval_f32: trc_core.h's production evaluation (double arithmetic around a pow cut to what a float result needs)
//   3 powf     the table in single precision around powf: misses the 1-ulp bar (up to 4 ulp), timed for the record
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../dspfun_amd/csrc/trc_core.h"

using namespace dspfft;

namespace {

__device__ float eval_powf(const TrcParams &p, int inverse, float v)
{
	const float a = (float)p.a, b = (float)p.b, s = (float)p.slope, g = (float)(inverse ? p.g_dec : p.g_enc);
	if (p.shape == 0) return v;
	if (p.shape == 1) return 0 > v ? 0.0f : powf(v, g);
	const float th = inverse ? s * b : b;
	if (p.shape == 3 && -th >= v) return inverse ? -powf((-v + (a - 1)) / a, g) : -(a * powf(-v, g) - (a - 1));
	if (p.shape == 2 && 0 > v) return 0.0f;
	if (th > v) return inverse ? v / s : s * v;
	return inverse ? powf((v + (a - 1)) / a, g) : a * powf(v, g) - (a - 1);
}

template <int CAND>
__device__ float eval(const TrcParams &p, int inverse, float v)
{
	if (CAND == 0) return v;
	if (CAND == 1) return (float)trc_exact(p, inverse, (double)v);
	if (CAND == 2) return trc_eval_f32(p, inverse, v);
	return eval_powf(p, inverse, v);
}

template <int CAND>
__global__ void __launch_bounds__(256) candidate_kernel(float *dst, const float *src, uint64_t nvec, int trc, int inverse)
{
	const TrcParams tp = trc_params(trc);
	const float4 *s4 = reinterpret_cast<const float4 *>(src);
	float4 *d4 = reinterpret_cast<float4 *>(dst);
	for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < nvec; i += gridDim.x * 256ull) {
		float4 v = s4[i];
		v.x = eval<CAND>(tp, inverse, v.x); v.y = eval<CAND>(tp, inverse, v.y);
		v.z = eval<CAND>(tp, inverse, v.z); v.w = eval<CAND>(tp, inverse, v.w);
		d4[i] = v;
	}
}

}  // namespace

// len a multiple of 4, both pointers 16-byte aligned
extern "C" int trc_candidate_apply(int cand, float *d_dst, const float *d_src, uint64_t len, int trc, int inverse, void *stream)
{
	if (len % 4 || ((uintptr_t)d_dst | (uintptr_t)d_src) & 15) return -1;
	const uint64_t nvec = len / 4, groups = (nvec + 255) / 256;
	const dim3 grid((unsigned)(groups < 1 ? 1 : groups > 8192 ? 8192 : groups));
	hipStream_t st = (hipStream_t)stream;
	switch (cand) {
	case 0: hipLaunchKernelGGL(candidate_kernel<0>, grid, dim3(256), 0, st, d_dst, d_src, nvec, trc, inverse); break;
	case 1: hipLaunchKernelGGL(candidate_kernel<1>, grid, dim3(256), 0, st, d_dst, d_src, nvec, trc, inverse); break;
	case 2: hipLaunchKernelGGL(candidate_kernel<2>, grid, dim3(256), 0, st, d_dst, d_src, nvec, trc, inverse); break;
	case 3: hipLaunchKernelGGL(candidate_kernel<3>, grid, dim3(256), 0, st, d_dst, d_src, nvec, trc, inverse); break;
	default: return -1;
	}
	return hipGetLastError() == hipSuccess ? 0 : -4;
}
