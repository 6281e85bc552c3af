// zoom_anim.hip -- the last pass of an animation frame (dspfft_zoomanim_execute): zoom's --showsamples overlay (zoom/zoom.c:377-390) and
// the GBRPF32 store (zoom.c:392-397 through ffapi_setpelf).  The per-pixel rule is zoom_anim_core.h's; this file only schedules pixels,
// one lane per output pixel, memory-bound.
//  * interleaved frame with the overlay: in place, only the marked pixels are written;
//  * planar (GBR) frame: reads the x stage's interleaved frame once and writes the three planes, the overlay applied on the way.
// zoom -g (a transfer characteristic, trc_core.h) encodes every sample after the overlay (zoom.c:392-399), the marker's (0, 1, 0) included:
// inside the planar store, and in place on the interleaved frame (za_encode_kernel, the overlay applied on the way).  Without it the
// launches and kernels are the ones above, unchanged.
// engine.cpp reaches the launcher through a weak reference: the CPU emulation build has no kernels and reports "not in this build".
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "zoom_anim_core.h"
#include "trc_core.h"

using namespace dspfft;

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) za_overlay_kernel(float *out, const ZaOverlay o)
{
	const long long npix = (long long)o.vw * o.vh;
	for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < npix; i += (long long)gridDim.x * kThreads)
		if (za_overlay_hit(o, i)) { out[3 * i] = 0.f; out[3 * i + 1] = 1.f; out[3 * i + 2] = 0.f; }
}

template <bool TRC>
__global__ void __launch_bounds__(kThreads) za_planar_kernel(float *out, const float *src, const ZaOverlay o, int trc)
{
	const long long npix = (long long)o.vw * o.vh;
	TrcParams tp;
	if (TRC) tp = trc_params(trc);
	for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < npix; i += (long long)gridDim.x * kThreads) {
		float v[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
		if (za_overlay_hit(o, i)) { v[0] = 0.f; v[1] = 1.f; v[2] = 0.f; }
		for (int z = 0; z < 3; z++) out[za_plane_of(z) * npix + i] = TRC ? trc_eval_f32(tp, 0, v[z]) : v[z];
	}
}

// the interleaved frame in place: overlay, then the encode
__global__ void __launch_bounds__(kThreads) za_encode_kernel(float *out, const ZaOverlay o, int trc)
{
	const long long npix = (long long)o.vw * o.vh;
	const TrcParams tp = trc_params(trc);
	for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < npix; i += (long long)gridDim.x * kThreads) {
		float v[3] = {out[3 * i], out[3 * i + 1], out[3 * i + 2]};
		if (za_overlay_hit(o, i)) { v[0] = 0.f; v[1] = 1.f; v[2] = 0.f; }
		for (int z = 0; z < 3; z++) out[3 * i + z] = trc_eval_f32(tp, 0, v[z]);
	}
}

}  // namespace

// d_out: the caller's frame (interleaved vh x vw x 3, or three vw x vh planes G, B, R); src: the x stage's interleaved frame (== d_out
// when interleaved)
extern "C" __attribute__((visibility("hidden"))) int dspfft_zoomanim_finish_launch(float *d_out, const float *src, const ZaOverlay *o, int planar,
                                                                                    int trc, void *stream, char *err, size_t errlen)
{
	const long long npix = (long long)o->vw * o->vh;
	const long long groups = (npix + kThreads - 1) / kThreads;
	const dim3 grid((unsigned)(groups < 8192 ? groups : 8192));
	if (planar && trc)
		hipLaunchKernelGGL(za_planar_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, d_out, src, *o, trc);
	else if (planar)
		hipLaunchKernelGGL(za_planar_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, d_out, src, *o, 0);
	else if (trc)
		hipLaunchKernelGGL(za_encode_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, d_out, *o, trc);
	else if (o->mode)
		hipLaunchKernelGGL(za_overlay_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, d_out, *o);
	else
		return 0;
	if (hipGetLastError() != hipSuccess) { snprintf(err, errlen, "zoom animation: kernel launch failed"); return -4; }
	return 0;
}
