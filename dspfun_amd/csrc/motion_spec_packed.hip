// motion_spec_packed.hip -- motion --spectrogram / --ispectrogram over full frames of PACKED 8-bit pixels (the reference's default block
// 0x0x1 on rgb24, bgr24, rgba ...: motion/motion.c:313-318): the encode and the decode of motion_ops.hip's motion_spec_blocks_kernel /
// motion_ispec_blocks_kernel on a dense [frames][h][w][C] layout that pixels and coefficients share element for element
// (dspfft_motion_spec_blocks_u8_packed, dspfft_motion_ispec_blocks_u8_packed; the pointwise end of dspfft_execute_spectrogram_u8_packed /
// _ispectrogram_u8_packed beside the passes of an interleaved plan).  Every component of a frame is a block of its own (:613-615): element e
// of a row belongs to component e mod C at x = e / C, abs takes a component's c from that component's DC at the frame's first pixel
// (:650,755), and damp, boost and grey_add are the component's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>

#include "../../include/dspfft.h"
#include "motion_filter.h"

extern "C" __attribute__((visibility("hidden"))) int dspfft_motion_set_error(const char *m);   // motion_ops.hip: dspfft_motion_last_error's text

namespace {
using namespace dspfft;

struct PackedFrames { uint32_t h, row, per; unsigned int frames; float damp[4], boost[4], grey_add[4]; };   // row = w C elements, per = h row

template <int C, class T>
__device__ inline T pick(const T (&v)[C], int c)
{
	T r = v[0];
#pragma unroll
	for (int k = 1; k < C; k++) r = c == k ? v[k] : r;
	return r;
}
template <int C>
__device__ inline MotionFilter filter_of(const MotionFilter &f, const PackedFrames &r, int c)
{
	MotionFilter g = f;
	float d = r.damp[0], b = r.boost[0], a = r.grey_add[0];
#pragma unroll
	for (int k = 1; k < C; k++) { d = c == k ? r.damp[k] : d; b = c == k ? r.boost[k] : b; a = c == k ? r.grey_add[k] : a; }
	g.damp = d; g.boost = b; g.grey_add = a;
	return g;
}
__device__ inline void coded_add(unsigned long long mine, unsigned long long *coded)
{
	unsigned int m = (unsigned int)mine;
	for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(coded, (unsigned long long)m);
}

// a thread takes W = 4 consecutive elements of a row (one dword of pixels, a float4 of coefficients) where rows are multiples of 4 elements and
// the buffers aligned, else one; frames along blockIdx.y, striding.  c is read only: the frame's first pixel still holds the C DCs.
template <int C, int W>
__global__ void __launch_bounds__(256) spec_frames_packed_kernel(uint8_t *pix, const float *c, PackedFrames r, MotionSpec sp, MotionFilter f, unsigned long long *coded)
{
	const uint32_t qx = r.row / W, per = r.h * qx;
	unsigned long long mine = 0;
	for (uint32_t b = blockIdx.y; b < r.frames; b += gridDim.y) {
		const float *cb = c + (size_t)b * r.per;
		uint8_t *pb = pix + (size_t)b * r.per;
		double cc[C];
		float fm[C], fcc[C];
		int fon[C];
#pragma unroll
		for (int k = 0; k < C; k++) {
			cc[k] = sp.mode == MOTION_MODE_ABS ? motion_abs_c(cb[k], sp.scalefactor, sp.norm) : sp.c;                      // :755
			const MotionFast t = motion_fast_of(sp.mode, sp.scalefactor, sp.norm, cc[k]);
			fm[k] = t.m; fcc[k] = t.cc; fon[k] = t.on;
		}
		for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x) {
			const uint32_t y = e / qx, i0 = (e - y * qx) * W;
			const size_t o = (size_t)y * r.row + i0;
			float v[W];
			if constexpr (W == 4) { const float4 t = *reinterpret_cast<const float4 *>(cb + o); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
			else v[0] = cb[o];
			uint32_t w4 = 0;
#pragma unroll
			for (int k = 0; k < W; k++) {
				const uint32_t x = (i0 + k) / C;
				const int comp = (int)(i0 + k - x * C);
				if (f.enabled && (int)x < f.aw && (int)y < f.ah && 0 < f.ad) v[k] = motion_filter_at(filter_of<C>(f, r, comp), 0, (int)y, (int)x, v[k], mine);
				MotionFast fast; fast.m = pick<C>(fm, comp); fast.cc = pick<C>(fcc, comp); fast.on = pick<C>(fon, comp);
				w4 |= motion_spec_byte(v[k], sp.mode, sp.scalefactor, sp.norm, pick<C>(cc, comp), fast) << (8 * k);             // :759-776
			}
			if constexpr (W == 4) *reinterpret_cast<uint32_t *>(pb + o) = w4; else pb[o] = (uint8_t)w4;
		}
	}
	if (coded && f.enabled) coded_add(mine, coded);
}
// bytes -> the coefficients they stand for (:621-637) -> filtered (:683-744)
template <int C, int W>
__global__ void __launch_bounds__(256) ispec_frames_packed_kernel(float *c, const uint8_t *pix, PackedFrames r, MotionSpec sp, MotionFilter f, unsigned long long *coded)
{
	const uint32_t qx = r.row / W, per = r.h * qx;
	unsigned long long mine = 0;
	for (uint32_t b = blockIdx.y; b < r.frames; b += gridDim.y) {
		float *cb = c + (size_t)b * r.per;
		const uint8_t *pb = pix + (size_t)b * r.per;
		for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x) {
			const uint32_t y = e / qx, i0 = (e - y * qx) * W;
			const size_t o = (size_t)y * r.row + i0;
			uint32_t w4;
			if constexpr (W == 4) w4 = *reinterpret_cast<const uint32_t *>(pb + o); else w4 = pb[o];
			float v[W];
#pragma unroll
			for (int k = 0; k < W; k++) {
				const uint32_t x = (i0 + k) / C;
				const int comp = (int)(i0 + k - x * C);
				v[k] = (float)motion_load_pel((double)((w4 >> (8 * k)) & 0xffu), sp.mode, sp.c, sp.norm);                      // :625-637
				if (f.enabled && (int)x < f.aw && (int)y < f.ah && 0 < f.ad) v[k] = motion_filter_at(filter_of<C>(f, r, comp), 0, (int)y, (int)x, v[k], mine);
			}
			if constexpr (W == 4) { float4 t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; *reinterpret_cast<float4 *>(cb + o) = t; }
			else cb[o] = v[0];
		}
	}
	if (coded && f.enabled) coded_add(mine, coded);
}

template <int C, int W>
void launch(bool inverse, uint8_t *pix, float *c, const PackedFrames &r, const MotionSpec &sp, const MotionFilter &f, unsigned long long *coded, hipStream_t s)
{
	const size_t per = (size_t)r.h * (r.row / W);
	const dim3 grid((unsigned)std::min<size_t>((per + 255) / 256, 4096), std::min(r.frames, 65535u));
	if (inverse) hipLaunchKernelGGL((ispec_frames_packed_kernel<C, W>), grid, dim3(256), 0, s, c, (const uint8_t *)pix, r, sp, f, coded);
	else hipLaunchKernelGGL((spec_frames_packed_kernel<C, W>), grid, dim3(256), 0, s, pix, (const float *)c, r, sp, f, coded);
}
template <int C>
void launch_c(bool inverse, bool vec, uint8_t *pix, float *c, const PackedFrames &r, const MotionSpec &sp, const MotionFilter &f, unsigned long long *coded, hipStream_t s)
{
	if (vec) launch<C, 4>(inverse, pix, c, r, sp, f, coded, s); else launch<C, 1>(inverse, pix, c, r, sp, f, coded, s);
}

int frames_call(bool inverse, uint8_t *d_pix, float *d_coeffs, int h, int w, int comps, size_t frames, const dspfft_motion_spec_params *spp,
                const dspfft_motion_filter_params *fp, const dspfft_motion_packed *packed, unsigned long long *d_coded, void *stream)
{
	if (!d_pix || !d_coeffs || !spp || !packed || h < 1 || w < 1 || !frames) return dspfft_motion_set_error("bad arguments");
	if (comps < 2 || comps > 4 || packed->components != comps) return dspfft_motion_set_error("components must be 2, 3 or 4 and equal packed->components");
	const int m = spp->mode;
	if (m < DSPFFT_MOTION_NONE || m > DSPFFT_MOTION_COPY || (inverse && m == DSPFFT_MOTION_ABS))
		return dspfft_motion_set_error(inverse ? "ispec mode: none, shift, flat or copy" : "spec mode: none, abs, shift, flat or copy");
	if ((unsigned long long)h * w * comps >= (1ull << 32) || frames >= (1ull << 32)) return dspfft_motion_set_error("a frame of 2^32 samples or more, or 2^32 frames or more");
	if (fp && (fp->preserve_dc < 0 || fp->preserve_dc > 2 || fp->minbuf_hw[0] < 1 || fp->minbuf_hw[1] < 1 || fp->block_depth < 1)) return dspfft_motion_set_error("bad filter parameters");
	MotionFilter f;
	memset((void *)&f, 0, sizeof f);
	if (fp) motion_filter_from(*fp, f);
	PackedFrames r;
	memset(&r, 0, sizeof r);
	r.h = (uint32_t)h; r.row = (uint32_t)w * comps; r.per = r.h * r.row; r.frames = (unsigned int)frames;
	if (fp) for (int k = 0; k < comps; k++) { r.damp[k] = packed->damp[k]; r.boost[k] = packed->boost[k]; r.grey_add[k] = packed->grey_add[k]; }
	const MotionSpec sp = {m, spp->scalefactor, spp->normalization, spp->c};
	const bool vec = r.row % 4 == 0 && !((uintptr_t)d_pix & 3u) && !((uintptr_t)d_coeffs & 15u);
	hipStream_t s = (hipStream_t)stream;
	switch (comps) {
	case 2: launch_c<2>(inverse, vec, d_pix, d_coeffs, r, sp, f, d_coded, s); break;
	case 3: launch_c<3>(inverse, vec, d_pix, d_coeffs, r, sp, f, d_coded, s); break;
	default: launch_c<4>(inverse, vec, d_pix, d_coeffs, r, sp, f, d_coded, s); break;
	}
	return hipGetLastError() == hipSuccess ? 0 : -4;
}
}  // namespace

extern "C" int dspfft_motion_spec_blocks_u8_packed(uint8_t *d_pix, const float *d_coeffs, int h, int w, int components, size_t frames, const dspfft_motion_spec_params *sp,
                                                   const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *stream)
{
	return frames_call(false, d_pix, (float *)d_coeffs, h, w, components, frames, sp, filter, packed, d_coeffs_coded, stream);
}
extern "C" int dspfft_motion_ispec_blocks_u8_packed(float *d_coeffs, const uint8_t *d_pix, int h, int w, int components, size_t frames, const dspfft_motion_spec_params *sp,
                                                    const dspfft_motion_filter_params *filter, const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *stream)
{
	return frames_call(true, (uint8_t *)d_pix, d_coeffs, h, w, components, frames, sp, filter, packed, d_coeffs_coded, stream);
}

/* the same for dspfft_execute_spectrogram_u8_packed / _ispectrogram_u8_packed (engine.cpp reaches this through a weak reference); the error
 * text is dspfft_motion_last_error's */
extern "C" __attribute__((visibility("hidden"))) int dspfft_spec_frames_packed_launch(int inverse, uint8_t *d_pix, float *d_coeffs, int h, int w, int components, size_t frames,
                                                                                       const dspfft_motion_spec_params *sp, const dspfft_motion_filter_params *filter,
                                                                                       const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *stream)
{
	return frames_call(inverse != 0, d_pix, d_coeffs, h, w, components, frames, sp, filter, packed, d_coeffs_coded, stream);
}
