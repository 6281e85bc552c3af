// spec_image.hip -- the two pointwise sweeps of dspfft_execute_spec_u8 / dspfft_execute_ispec_u8 (include/dspfft.h; the sample arithmetic is
// spec_image_core.h's):
//   encode + store  float coefficients -> spectrogram bytes, and in the same sweep the `sign` preset's bytes (the sign map of ispec -m) and
//                   the DC doubles of the header: 4 B read and 1 (2) B written per sample, where dspfft_spec_encode + dspfft_f32_to_u8
//                   move 13 and run twice for the sign map.  The float buffer is only read, so every lane derives the divisors from the
//                   first pixel itself: one launch, no scratch, no allocation.
//   load + decode   spectrogram bytes (+ sign map) -> float coefficients: 1 (2) B read and 4 B written per sample, against 20 (29).
// A lane moves four consecutive samples: a 16-byte float access and a dword of bytes, where the buffers are aligned for it; the scalar form
// takes any alignment.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "spec_image_core.h"

namespace {
using namespace dspfft;

// VEC: a.f is 16-byte aligned and the byte buffers 4-byte aligned; groups of four samples, the tail of len % 4 samples one per lane
template <bool VEC>
__global__ void __launch_bounds__(256) spec_image_encode_kernel(const SpecImageEnc a)
{
	float m[SPEC_IMAGE_MAX_CH];
	spec_image_divisors(m, a.f, a.d, a.gain, a.rangetype, a.scaletype);
	const uint64_t tid = blockIdx.x * 256ull + threadIdx.x, stride = gridDim.x * 256ull;
	if (a.dc && tid < (uint64_t)a.d) a.dc[tid] = (double)a.f[tid];                      // spec.c:66-68
	const uint64_t nvec = VEC ? a.len / 4 : 0;
	for (uint64_t g = tid; g < nvec; g += stride) {
		const float4 v = reinterpret_cast<const float4 *>(a.f)[g];
		const float f4[4] = {v.x, v.y, v.z, v.w};
		int z = (int)((4 * g) % (uint64_t)a.d);
		uint32_t w = 0, s = 0;
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const bool first = 4 * g + q < (uint64_t)a.d;
			w |= (uint32_t)spec_image_byte(spec_image_encode(f4[q], first, m[z], a.gain, a.scaletype, a.signtype)) << (8 * q);
			s |= (uint32_t)spec_image_sign_byte(f4[q], first) << (8 * q);
			if (++z == a.d) z = 0;
		}
		reinterpret_cast<uint32_t *>(a.out)[g] = w;
		if (a.signmap) reinterpret_cast<uint32_t *>(a.signmap)[g] = s;
	}
	for (uint64_t i = 4 * nvec + tid; i < a.len; i += stride) {
		uint8_t b, sb;
		spec_image_encode_at(a, m, i, (int)(i % (uint64_t)a.d), b, sb);
		a.out[i] = b;
		if (a.signmap) a.signmap[i] = sb;
	}
}

template <bool VEC>
__global__ void __launch_bounds__(256) spec_image_decode_kernel(const SpecImageDec a)
{
	const uint64_t tid = blockIdx.x * 256ull + threadIdx.x, stride = gridDim.x * 256ull;
	const uint64_t nvec = VEC ? a.len / 4 : 0;
	for (uint64_t g = tid; g < nvec; g += stride) {
		const uint32_t w = reinterpret_cast<const uint32_t *>(a.in)[g];
		const uint32_t s = a.signmap ? reinterpret_cast<const uint32_t *>(a.signmap)[g] : 0u;
		int z = (int)((4 * g) % (uint64_t)a.d);
		float o[4];
#pragma unroll
		for (int q = 0; q < 4; q++) {
			o[q] = spec_image_decode_at(a, 4 * g + q, z, (uint8_t)(w >> (8 * q)), (uint8_t)(s >> (8 * q)));
			if (++z == a.d) z = 0;
		}
		reinterpret_cast<float4 *>(a.f)[g] = make_float4(o[0], o[1], o[2], o[3]);
	}
	for (uint64_t i = 4 * nvec + tid; i < a.len; i += stride)
		a.f[i] = spec_image_decode_at(a, i, (int)(i % (uint64_t)a.d), a.in[i], a.signmap ? a.signmap[i] : (uint8_t)0);
}

inline int grid_for(uint64_t n) { const uint64_t b = (n + 255) / 256; return (int)(b < 1 ? 1 : b > 8192 ? 8192 : b); }
inline bool aligned(const void *p, uintptr_t n) { return !((uintptr_t)p & (n - 1)); }

}  // namespace

/* the sweeps' launchers (engine.cpp has checked the arguments and reaches these through weak references: the CPU emulation links engine.cpp
 * without this unit) */
extern "C" __attribute__((visibility("hidden"))) int dspfft_spec_image_encode_launch(const dspfft::SpecImageEnc *a, void *stream)
{
	const bool vec = aligned(a->f, 16) && aligned(a->out, 4) && (!a->signmap || aligned(a->signmap, 4));
	const int grid = grid_for(vec ? (a->len + 3) / 4 : a->len);
	if (vec) hipLaunchKernelGGL(spec_image_encode_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
	else hipLaunchKernelGGL(spec_image_encode_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}
extern "C" __attribute__((visibility("hidden"))) int dspfft_spec_image_decode_launch(const dspfft::SpecImageDec *a, void *stream)
{
	const bool vec = aligned(a->f, 16) && aligned(a->in, 4) && (!a->signmap || aligned(a->signmap, 4));
	const int grid = grid_for(vec ? (a->len + 3) / 4 : a->len);
	if (vec) hipLaunchKernelGGL(spec_image_decode_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
	else hipLaunchKernelGGL(spec_image_decode_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}
