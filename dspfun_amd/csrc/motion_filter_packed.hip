// motion_filter_packed.hip -- motion's coefficient filter (motion/motion.c:683-744) over full frames of PACKED pixels, as a pointwise kernel
// on a dense [frames][h][w][C] buffer of coefficients: dspfft_motion_filter_packed, what dspfft_motion_filter is for planar buffers, and the
// unfused middle step of dspfft_execute_roundtrip_u8_packed_frames.  Every component of a frame is a block of its own (:613-615): element e of
// a row belongs to component e mod C at x = e / C, and damp, boost and grey_add are the component's (motion_filter_packed.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>

#include "../../include/dspfft.h"
#include "motion_filter_packed.h"

extern "C" __attribute__((visibility("hidden"))) int dspfft_motion_set_error(const char *m);   // motion_ops.hip: dspfft_motion_last_error's text

namespace {
using namespace dspfft;

// a thread takes W = 4 consecutive elements of a row (a float4) where rows are multiples of 4 elements and the buffer is 16-byte aligned, else
// one; frames along blockIdx.y, striding, so that every offset a thread forms is frame-local (< 2^32)
template <int W>
__global__ void __launch_bounds__(256) motion_filter_packed_kernel(float *c, MotionFilterPacked p, unsigned int frames, unsigned long long *coded)
{
	const uint32_t qx = p.row / W;
	const size_t n = (size_t)p.h * qx;
	unsigned long long mine = 0;
	for (uint32_t b = blockIdx.y; b < frames; b += gridDim.y) {
		float *cb = c + (size_t)b * p.per;
		for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
			const uint32_t y = (uint32_t)e / qx, i0 = ((uint32_t)e - y * qx) * W;
			const size_t o = (size_t)y * p.row + i0;
			if constexpr (W == 4) {
				float4 *at = reinterpret_cast<float4 *>(cb + o);
				*at = motion_filter_packed4_at(p, y, i0, *at, mine);
			} else cb[o] = motion_filter_packed_elem(p, y, i0, cb[o], mine);
		}
	}
	if (coded) {          // one atomic per wave
		unsigned int m = (unsigned int)mine;
		for (int off = 32; off > 0; off >>= 1) m += __shfl_xor(m, off);
		if ((threadIdx.x & 63) == 0 && m) atomicAdd(coded, (unsigned long long)m);
	}
}
}  // namespace

extern "C" int dspfft_motion_filter_packed(float *d_coeffs, int h, int w, int components, size_t frames, const dspfft_motion_filter_params *fp,
                                           const dspfft_motion_packed *packed, unsigned long long *d_coeffs_coded, void *stream)
{
	if (!d_coeffs || !fp || !packed || h < 1 || w < 1 || !frames) return dspfft_motion_set_error("bad arguments");
	if (components < 2 || components > 4 || packed->components != components) return dspfft_motion_set_error("components must be 2, 3 or 4 and equal packed->components");
	if ((unsigned long long)h * w * components >= (1ull << 32) || frames >= (1ull << 32)) return dspfft_motion_set_error("a frame of 2^32 samples or more, or 2^32 frames or more");
	if (fp->preserve_dc < 0 || fp->preserve_dc > 2 || fp->minbuf_hw[0] < 1 || fp->minbuf_hw[1] < 1 || fp->block_depth < 1) return dspfft_motion_set_error("bad filter parameters");
	MotionFilter f;
	memset((void *)&f, 0, sizeof f);
	motion_filter_from(*fp, f);
	MotionFilterPacked p;
	memset((void *)&p, 0, sizeof p);
	motion_filter_packed_set(p, f, h, w, components, packed->damp, packed->boost, packed->grey_add);
	const bool vec = p.row % 4 == 0 && !((uintptr_t)d_coeffs & 15u);
	const size_t n = (size_t)h * (p.row / (vec ? 4 : 1));
	const dim3 grid((unsigned)std::min<size_t>((n + 255) / 256, 4096), (unsigned)std::min<size_t>(frames, 65535));
	if (vec) hipLaunchKernelGGL(motion_filter_packed_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, d_coeffs, p, (unsigned int)frames, d_coeffs_coded);
	else hipLaunchKernelGGL(motion_filter_packed_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, d_coeffs, p, (unsigned int)frames, d_coeffs_coded);
	return hipGetLastError() == hipSuccess ? 0 : -4;
}
