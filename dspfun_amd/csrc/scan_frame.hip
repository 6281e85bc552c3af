// scan_frame.hip -- scan's output frame composed on the device (scan/scan.c:379-417 clear and fill, :419-527 the loop's panels and
// parity).  The per-pixel arithmetic is scan_frame_core.h's; this file only schedules pixels.  Every kernel is one lane per pixel (or per
// coordinate slot) and memory-bound; frame offsets are 64-bit.
//  * mark: lights the top-right panel (and, for the current frame with -i, the bottom-right one) at the pixels of a set of scan indices:
//    an owner-index range [lo, hi) (one pass over the index table, which also clears the previous frame's bottom-right marks), or a
//    coordinate list (box, files whose indices share pixels).
//  * compose, per frame: sum += image (with -i), the reconstruction and intermediates panels, -P's comparison.  -M first reduces the
//    frame's inverse to per-workgroup (value, index) extremes and finishes them in one workgroup: exact, and independent of the order the
//    parts combine in (no float atomics).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdio.h>
#include <string.h>

#include "scan_frame_core.h"
#include "trc_core.h"

using namespace dspfft;

namespace {

constexpr int kThreads = 256;
constexpr int kReduceGroups = 1024;     // -M partials: per workgroup and channel, min / max value and index
constexpr float kNegZero = -0.0f;

struct Extremes { float mn[3], mx[3]; uint32_t imn[3], imx[3]; };

__global__ void __launch_bounds__(64) sf_begin_kernel(SfState *st, const float *coeffs, int scaletype, int signtype, double gain)
{
	if (threadIdx.x) return;
	const SfScaler s = sf_scaler(scaletype, signtype, gain, coeffs[0], coeffs[1], coeffs[2]);
	st->gain = s.gain; st->max = s.max;
	for (int z = 0; z < 3; z++) { st->mn[z] = 0.0f; st->mx[z] = 1.0f; }
	st->reached = 0; st->parity_frame = ~0ull;
}

DSP_HD SfScaler scaler_of(const SfState *st, int scaletype, int signtype)
{
	SfScaler s;
	s.gain = st->gain; s.max = st->max; s.scaletype = scaletype; s.signtype = signtype;
	return s;
}

// one lane per pixel: owner index in [lo, hi) -> light; else in [clo, chi) -> clear the bottom-right mark
__global__ void __launch_bounds__(kThreads) sf_mark_range_kernel(SfOp o)
{
	const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
	const uint64_t npix = (uint64_t)o.w * o.h;
	if (p >= npix) return;
	const uint32_t id = o.owner[p];
	const bool lit = id - o.lo < o.hi - o.lo;
	const bool clr = !lit && o.bottom && id - o.clo < o.chi - o.clo;
	if (!lit && !clr) return;
	const uint32_t y = (uint32_t)(p / o.w), x = (uint32_t)(p - (uint64_t)y * o.w);
	const uint64_t fw = 2ull * o.w, fh = (uint64_t)o.h * (1 + (o.intermediates != 0));
	if (clr) {
		for (int z = 0; z < 3; z++) o.frame[sf_frame_offset(fw, fh, x + o.w, y + o.h, z)] = 0.0f;
		return;
	}
	const SfScaler s = scaler_of(o.state, o.scaletype, o.signtype);
	for (int z = 0; z < 3; z++) {
		const float v = sf_mark_value(o.spectrogram, s, o.coeffs[p * 3 + z], x, y);
		if (o.top) o.frame[sf_frame_offset(fw, fh, x + o.w, y, z)] = v;
		if (o.bottom) o.frame[sf_frame_offset(fw, fh, x + o.w, y + o.h, z)] = v;
	}
}

// one lane per slot of a y*w+x list; top = bottom = 0: clear the bottom-right panel there
__global__ void __launch_bounds__(kThreads) sf_mark_coords_kernel(SfOp o)
{
	const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
	if (k >= o.nslots) return;
	const uint32_t p = o.lin[k];
	if (p == 0xFFFFFFFFu || (uint64_t)p >= (uint64_t)o.w * o.h) return;
	const uint32_t y = p / o.w, x = p - y * o.w;
	const uint64_t fw = 2ull * o.w, fh = (uint64_t)o.h * (1 + (o.intermediates != 0));
	if (!o.top && !o.bottom) {
		for (int z = 0; z < 3; z++) o.frame[sf_frame_offset(fw, fh, x + o.w, y + o.h, z)] = 0.0f;
		return;
	}
	const SfScaler s = scaler_of(o.state, o.scaletype, o.signtype);
	for (int z = 0; z < 3; z++) {
		const float v = sf_mark_value(o.spectrogram, s, o.coeffs[(uint64_t)p * 3 + z], x, y);
		if (o.top) o.frame[sf_frame_offset(fw, fh, x + o.w, y, z)] = v;
		if (o.bottom) o.frame[sf_frame_offset(fw, fh, x + o.w, y + o.h, z)] = v;
	}
}

__device__ void merge(Extremes &a, const Extremes &b)
{
	for (int z = 0; z < 3; z++) {
		if (sf_min_wins(b.mn[z], b.imn[z], a.mn[z], a.imn[z])) { a.mn[z] = b.mn[z]; a.imn[z] = b.imn[z]; }
		if (sf_max_wins(b.mx[z], b.imx[z], a.mx[z], a.imx[z])) { a.mx[z] = b.mx[z]; a.imx[z] = b.imx[z]; }
	}
}
__device__ void empty(Extremes &e)
{
	for (int z = 0; z < 3; z++) { e.mn[z] = INFINITY; e.mx[z] = -INFINITY; e.imn[z] = e.imx[z] = 0xFFFFFFFFu; }
}
// workgroup-wide merge through LDS; lane 0 returns the result
__device__ Extremes block_merge(Extremes e)
{
	__shared__ Extremes sh[kThreads];
	sh[threadIdx.x] = e;
	__syncthreads();
	for (int s = kThreads / 2; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) { Extremes a = sh[threadIdx.x]; merge(a, sh[threadIdx.x + s]); sh[threadIdx.x] = a; }
		__syncthreads();
	}
	return sh[0];
}

// -M, pass 1: every workgroup strides over the pixels in raster order (strict comparisons keep the first of equal values per lane)
__global__ void __launch_bounds__(kThreads) sf_reduce_kernel(const float *image, uint64_t npix, Extremes *part)
{
	Extremes e;
	empty(e);
	for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < npix; p += (uint64_t)gridDim.x * kThreads)
		for (int z = 0; z < 3; z++) {
			const float c = image[p * 3 + z];
			if (c < e.mn[z] || e.imn[z] == 0xFFFFFFFFu) { e.mn[z] = c; e.imn[z] = (uint32_t)p; }
			if (c > e.mx[z] || e.imx[z] == 0xFFFFFFFFu) { e.mx[z] = c; e.imx[z] = (uint32_t)p; }
		}
	const Extremes r = block_merge(e);
	if (threadIdx.x == 0) part[blockIdx.x] = r;
}
// -M, pass 2: one workgroup; min / max plus DC (scan.c:475-478)
__global__ void __launch_bounds__(kThreads) sf_reduce_finish_kernel(const Extremes *part, int nparts, const float *coeffs, SfState *st)
{
	Extremes e;
	empty(e);
	for (int i = threadIdx.x; i < nparts; i += kThreads) merge(e, part[i]);
	const Extremes r = block_merge(e);
	if (threadIdx.x == 0)
		for (int z = 0; z < 3; z++) {
			SF_NO_CONTRACT
			st->mx[z] = r.mx[z] + coeffs[z];
			st->mn[z] = r.mn[z] + coeffs[z];
		}
}

// one lane per pixel: sum (+= image), the top-left and bottom-left panels, image back to -0, -P's comparison.  TRC (scan -g): what goes
// into the two panels is encoded (scan.c:412-414,455-457,486-488: only `pel`); the sum, -P and -M stay linear.  Without it the kernel is
// the one it was: no extra arithmetic, the same stores.
template <bool TRC>
__global__ void __launch_bounds__(kThreads) sf_compose_kernel(SfOp o)
{
	SF_NO_CONTRACT
	const uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
	const uint64_t npix = (uint64_t)o.w * o.h;
	bool differs = false;
	const bool check = o.original && !o.state->reached;
	if (p < npix) {
		const uint32_t y = (uint32_t)(p / o.w), x = (uint32_t)(p - (uint64_t)y * o.w);
		const uint64_t fw = (uint64_t)o.w * (1 + (o.visualize != 0)), fh = (uint64_t)o.h * (1 + (o.intermediates != 0));
		float s[3], im[3];
		TrcParams tp;
		if (TRC) tp = trc_params(o.trc);
		for (int z = 0; z < 3; z++) s[z] = o.sum[p * 3 + z];
		if (o.image) {
			for (int z = 0; z < 3; z++) { im[z] = o.image[p * 3 + z]; s[z] += im[z]; }
			for (int z = 0; z < 3; z++) { o.sum[p * 3 + z] = s[z]; o.image[p * 3 + z] = kNegZero; }
		}
		for (int z = 0; z < 3; z++) o.frame[sf_frame_offset(fw, fh, x, y, z)] = TRC ? trc_eval_f32(tp, 0, s[z]) : s[z];
		if (o.intermediates && o.image)
			for (int z = 0; z < 3; z++) {
				const float v = sf_intermediate(im[z], o.coeffs[z], o.state->mn[z], o.state->mx[z]);
				o.frame[sf_frame_offset(fw, fh, x, y + o.h, z)] = TRC ? trc_eval_f32(tp, 0, v) : v;
			}
		if (check)
			for (int z = 0; z < 3; z++) differs |= sf_parity_differs(o.original[p * 3 + z], s[z], o.parity_depth);
	}
	// one flag per workgroup (distinct addresses: a single flag stored by every wave serialises them, 18 ms per 8K frame)
	if (check) {
		const int any = __syncthreads_or(differs);
		if (threadIdx.x == 0) o.flags[blockIdx.x] = any;
	}
}

// -P: one workgroup ORs the compose workgroups' flags; the first frame with none set is at parity
__global__ void __launch_bounds__(kThreads) sf_parity_finish_kernel(SfState *st, const uint32_t *flags, uint32_t nflags, uint64_t frame_no)
{
	if (st->reached) return;
	uint32_t any = 0;
	for (uint32_t i = threadIdx.x; i < nflags; i += kThreads) any |= flags[i];
	if (__syncthreads_or(any)) return;
	if (threadIdx.x == 0) { st->reached = 1; st->parity_frame = frame_no; }
}

int bad(char *err, size_t len, const char *m) { if (err && len) snprintf(err, len, "%s", m); return -1; }
unsigned groups(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

// The launcher behind the dspfft_scanframes_* entry points (engine.cpp reaches it through a weak reference: absent from the CPU emulation
// build).  engine.cpp has checked the arguments.
extern "C" __attribute__((visibility("hidden"))) int dspfft_scanframes_launch(SfOp *o, char *err, size_t errlen)
{
	hipStream_t st = (hipStream_t)o->stream;
	const uint64_t npix = (uint64_t)o->w * o->h;
	const uint64_t fw = (uint64_t)o->w * (1 + (o->visualize != 0)), fh = (uint64_t)o->h * (1 + (o->intermediates != 0));
	if (npix / kThreads >= 0xFFFFFFFFull) return bad(err, errlen, "scan frames: image too large");
	switch (o->op) {
	case SF_OP_ALLOC:
		if (hipMalloc((void **)&o->state, sizeof(SfState)) != hipSuccess) return bad(err, errlen, "scan frames: out of device memory");
		if (hipMemset(o->state, 0, sizeof(SfState)) != hipSuccess) return bad(err, errlen, "scan frames: memset failed");
		if ((o->max_intermediates && hipMalloc(&o->partials, kReduceGroups * sizeof(Extremes)) != hipSuccess) ||
		    (o->parity_depth && hipMalloc((void **)&o->flags, (size_t)groups(npix) * 4) != hipSuccess)) {
			(void)hipFree(o->state); (void)hipFree(o->partials); o->state = nullptr; o->partials = nullptr;
			return bad(err, errlen, "scan frames: out of device memory");
		}
		return 0;
	case SF_OP_FREE:
		(void)hipFree(o->state); (void)hipFree(o->partials); (void)hipFree(o->flags);
		if (o->saved) (void)hipFree(*o->saved);
		return 0;
	case SF_OP_BEGIN:
		if (hipMemsetAsync(o->frame, 0, 3 * fw * fh * sizeof(float), st) != hipSuccess) return bad(err, errlen, "scan frames: clear failed");
		hipLaunchKernelGGL(sf_begin_kernel, dim3(1), dim3(64), 0, st, o->state, o->coeffs, o->scaletype, o->signtype, o->gain);
		break;
	case SF_OP_MARK_RANGE:
		hipLaunchKernelGGL(sf_mark_range_kernel, dim3(groups(npix)), dim3(kThreads), 0, st, *o);
		break;
	case SF_OP_MARK_COORDS:
		if (!o->nslots) return 0;
		if (o->nslots / kThreads >= 0xFFFFFFFFull) return bad(err, errlen, "scan frames: coordinate list too long");
		hipLaunchKernelGGL(sf_mark_coords_kernel, dim3(groups(o->nslots)), dim3(kThreads), 0, st, *o);
		break;
	case SF_OP_SAVE_COORDS:
		if (o->nslots > *o->saved_cap) {
			(void)hipFree(*o->saved);       // synchronises the device: only while the list grows
			*o->saved = nullptr; *o->saved_cap = 0;
			if (hipMalloc((void **)o->saved, o->nslots * 4) != hipSuccess) return bad(err, errlen, "scan frames: out of device memory");
			*o->saved_cap = o->nslots;
		}
		if (o->nslots && hipMemcpyAsync(*o->saved, o->lin, o->nslots * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
			return bad(err, errlen, "scan frames: copy failed");
		return 0;
	case SF_OP_COMPOSE:
		if (o->max_intermediates && o->image) {
			const unsigned g = (unsigned)std::min<uint64_t>(kReduceGroups, groups(npix));
			hipLaunchKernelGGL(sf_reduce_kernel, dim3(g), dim3(kThreads), 0, st, o->image, npix, (Extremes *)o->partials);
			hipLaunchKernelGGL(sf_reduce_finish_kernel, dim3(1), dim3(kThreads), 0, st, (const Extremes *)o->partials, (int)g, o->coeffs, o->state);
		}
		if (o->trc) hipLaunchKernelGGL(sf_compose_kernel<true>, dim3(groups(npix)), dim3(kThreads), 0, st, *o);
		else hipLaunchKernelGGL(sf_compose_kernel<false>, dim3(groups(npix)), dim3(kThreads), 0, st, *o);
		if (o->original) hipLaunchKernelGGL(sf_parity_finish_kernel, dim3(1), dim3(kThreads), 0, st, o->state, (const uint32_t *)o->flags, groups(npix), o->frame_no);
		break;
	case SF_OP_PARITY:
		if (hipMemcpyAsync(o->parity_out, &o->state->parity_frame, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
			return bad(err, errlen, "scan frames: reading the parity frame failed");
		return 0;
	default:
		return bad(err, errlen, "scan frames: unknown operation");
	}
	return hipGetLastError() == hipSuccess ? 0 : bad(err, errlen, "scan frames: kernel launch failed");
}
